"""numpy restatement of the reverse walk's rule for ended problems (include/cmpc.h, cmpc_rollout_walk_vjp_device) and a made-up tick VJP
to drive it with.  For problem b let e = end_tick[b], -1 read as never; tick i is a good tick when e < 0 or i < e:

    c_i = [i < e] J_i^T c_{i+1} + [i <= e] G_i,        list carry_i = [i < e] (the tick's dGradPrevList),
    wrench row_i = gradP row_i = 0 and status_i = 6 for i >= e,

and for i >= e the tick is fed a zero state carry, a zero list carry, a zero dGradX row and ok = 0.  Everything is a selection (np.where), never a product
with a mask: what the tick leaves for an ended problem may be NaN."""
import numpy as np

SENS = 8


def ended(e, tick):
    return (e >= 0) & (tick >= e)


class FakeTick:
    """A made-up linear tick VJP, elementwise so that float64 results do not depend on a summation order:
        state = a_i * carry_state + gx[:, :9],  list = l_i * carry_list + gx[:, 9:9 + 6 M],  sens word 0 = a random status, wrench and gradP rows random.
    plant_nan: a problem fed ok = 0 (which is how the gate marks an ended one) gets NaN in every output -- the gate must select them away."""

    def __init__(self, T, B, M, N, nx, np_, seed, plant_nan=True):
        rng = np.random.default_rng(seed)
        self.a = rng.uniform(0.5, 1.5, (T, B, 9))
        self.l = rng.uniform(0.5, 1.5, (T, B, 2, M, 3))
        self.sens = rng.normal(size=(T, B, SENS)).astype(np.float32)
        self.sens[:, :, 0] = rng.integers(0, 5, (T, B))
        self.wrench = rng.normal(size=(T, B, N, 6)).astype(np.float32)
        self.gp = rng.normal(size=(T, B, np_)).astype(np.float32)
        self.M, self.plant_nan = M, plant_nan

    def __call__(self, i, carry_state, carry_list, gx, ok):
        B, M = carry_state.shape[0], self.M
        g9 = gx[:, :9].astype(np.float64) if gx is not None else 0.0
        g6 = gx[:, 9:9 + 6 * M].astype(np.float64).reshape(B, 2, M, 3) if gx is not None else 0.0
        out = dict(state=self.a[i] * carry_state + g9, list=self.l[i] * carry_list + g6, sens=self.sens[i].copy(), wrench=self.wrench[i].copy(),
                   gp=self.gp[i].copy())
        if self.plant_nan:
            for v in out.values():
                v[ok == 0] = np.nan
        return out


def reverse_walk(tick, e, tick0, ticks, row0, G, GX, ok, carry_state, carry_list):
    """rows row0 .. row0 + ticks - 1 in reverse under the rule; tick = a FakeTick.  -> dict(state, list: the carries leaving the first row; wrench, gp,
    status: the rows written, by row; fed: what each tick was given)"""
    B = G.shape[1]
    c, cl = carry_state.copy(), carry_list.copy()
    out = dict(wrench={}, gp={}, status={}, fed={})
    for i in reversed(range(ticks)):
        t, r = tick0 + i, row0 + i
        en = ended(e, t)
        # what the tick is fed: zeros and ok = 0 where the problem has ended
        f_c = np.where(en[:, None], 0.0, c)
        f_cl = np.where(en[:, None, None, None], 0.0, cl)
        f_gx = None if GX is None else np.where(en[:, None], np.float32(0), GX[r])
        f_ok = np.where(en, 0, ok[r]).astype(np.int32)
        out["fed"][r] = (f_c, f_cl, f_gx, f_ok)
        o = tick(r, f_c, f_cl, f_gx, f_ok)
        at_end = (e == t)
        c = np.where(en[:, None], np.where(at_end[:, None], G[r], 0.0), o["state"] + G[r])
        cl = np.where(en[:, None, None, None], 0.0, o["list"])
        out["wrench"][r] = np.where(en[:, None, None], np.float32(0), o["wrench"])
        out["gp"][r] = np.where(en[:, None], np.float32(0), o["gp"])
        out["status"][r] = np.where(en, 6, np.where(en, 0, o["sens"][:, 0]).astype(np.int32)).astype(np.int32)
    out["state"], out["list"] = c, cl
    return out


def closed_form_state0(tick, e, T, G, GX):
    """c_0 of a whole walk straight from the loss: sum over the states s_0 .. s_e of the seed carried back through the good ticks, plus the seeds on the
    solutions of the good ticks -- an independent statement of the carry rule (float64; agrees with the recursion to rounding)"""
    B = G.shape[1]
    out = np.zeros((B, 9))
    for b in range(B):
        last = T if e[b] < 0 else min(int(e[b]), T)      # the states 0 .. last exist
        for i in range(last + 1):
            v = G[i, b].copy()
            for j in reversed(range(i)):
                v = tick.a[j, b] * v
            out[b] += v
        if GX is not None:
            for i in range(last):                          # solutions of the good ticks i < e
                v = GX[i, b, :9].astype(np.float64)
                for j in reversed(range(i)):
                    v = tick.a[j, b] * v
                out[b] += v
    return out
