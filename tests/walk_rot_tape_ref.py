"""numpy restatement of the reverse walk's rule for ended problems with the orientation arrays (include/cmpc.h, cmpc_rollout_walk_vjp_rot_device; DESIGN.md
7f) and the made-up tick of tests/walk_tape_ref.py with orientation coefficients added, in both modes.  For problem b let e = end_tick[b], -1 read as never:

    l_rot_i = [i < e] (the tick's dGradPrevListRot),    row i of dGradRot = [i < e] (the tick's),    removed_i = [i < e] (word 6 of the tick's dTickSens),

next to the rule of walk_tape_ref for the state carry, the position carry, the wrench and gradP rows and the status; the first gate step of a call selects
zero in all three carries of an ended problem.  Everything is a selection (np.where), never a product with a mask."""
import numpy as np

from tests.walk_tape_ref import FakeTick, ended


def _sel(en, a):
    """zero where the problem has ended; en[B] against a[B, ...]"""
    return np.where(en.reshape((-1,) + (1,) * (a.ndim - 1)), a.dtype.type(0), a)


def gate_post(e, tick_post, seed, o, rows):
    """what the tick left (o: state, list, list_rot, sens) and the rows it wrote (rows: wrench, gp, rot -- any may be None) -> dict(state, list, list_rot:
    the carries; wrench, gp, rot: the rows gated; status, removed)"""
    en, at_end = ended(e, tick_post), e == tick_post
    out = dict(state=np.where(en[:, None], np.where(at_end[:, None], seed, 0.0), o["state"] + seed), list=_sel(en, o["list"]),
               list_rot=_sel(en, o["list_rot"]))
    for k in ("wrench", "gp", "rot"):
        out[k] = None if rows.get(k) is None else _sel(en, rows[k])
    out["status"] = np.where(en, 6, np.where(en, np.float32(0), o["sens"][:, 0]).astype(np.int32)).astype(np.int32)
    out["removed"] = np.where(en, np.float32(0), o["sens"][:, 6]).astype(np.float32)
    return out


def gate_pre(e, tick_pre, ok_row, gx_row, first, state, lst, lst_rot):
    """-> ok_out, gx_out (None without seeds on x) and the three carries: with `first` zero where the problem has ended at tick_pre, else as they came"""
    en = ended(e, tick_pre)
    ok_out = np.where(en, 0, ok_row if ok_row is not None else 1).astype(np.int32)
    gx_out = None if gx_row is None else _sel(en, gx_row)
    if first:
        state, lst, lst_rot = _sel(en, state), _sel(en, lst), _sel(en, lst_rot)
    return ok_out, gx_out, state, lst, lst_rot


class FakeTickRot:
    """walk_tape_ref.FakeTick with an orientation chain, still elementwise.  With c, cl, cr the carries that come in (state, positions, orientations):
        state = a_i * c + gx[:, :9],    list = l_i * cl + gx[:, 9:9 + 6 M]                      (FakeTick's)
        list_rot = lr_i * cr, and its first 9 entries also take q_i * c                          (the orientations move the state)
        plan += p_i * cl,    plan_rot += pr_i * cr                                               (what the merge sends to the planner's contacts)
        rot row: random [B, 2, N, 3];  sens word 6: random
    A problem fed ok = 0 adds nothing to plan / plan_rot (as the real tick) and, with plant_nan, gets NaN in every other output."""

    def __init__(self, T, B, M, N, nx, np_, seed, plant_nan=True):
        assert 6 * M >= 9
        self.f = FakeTick(T, B, M, N, nx, np_, seed, plant_nan=False)
        rng = np.random.default_rng(seed + 100)
        self.lr = rng.uniform(0.5, 1.5, (T, B, 2, M, 3))
        self.q = rng.uniform(-1.0, 1.0, (T, B, 9))
        self.p = rng.uniform(-1.0, 1.0, (T, B, 2, M, 3))
        self.pr = rng.uniform(-1.0, 1.0, (T, B, 2, M, 3))
        self.rot = rng.normal(size=(T, B, 2, N, 3))
        self.f.sens[:, :, 6] = rng.uniform(0.0, 1.0, (T, B)).astype(np.float32)
        self.M, self.plant_nan = M, plant_nan

    def __call__(self, i, c, cl, cr, gx, ok):
        B = c.shape[0]
        o = self.f(i, c, cl, gx, ok)
        lr = (self.lr[i] * cr).reshape(B, -1)
        lr[:, :9] = lr[:, :9] + self.q[i] * c
        o["list_rot"], o["rot"] = lr.reshape(cr.shape), self.rot[i].copy()
        good = (ok != 0)[:, None, None, None]
        o["plan_add"], o["plan_rot_add"] = np.where(good, self.p[i] * cl, 0.0), np.where(good, self.pr[i] * cr, 0.0)
        if self.plant_nan:
            for k, v in o.items():
                if k not in ("plan_add", "plan_rot_add"):
                    v[ok == 0] = np.nan
        return o


class FakeTickRotJvp:
    """The transpose of FakeTickRot, coefficient for coefficient; t, dl, dlr the directions that come in, dpl, dplr the planner's (constant over the walk):
        state' = a_i * t + q_i * dlr[:9],    list' = l_i * dl + p_i * dpl,    list_rot' = lr_i * dlr + pr_i * dplr,    dx[:9] = t,  dx[9:9 + 6 M] = dl
    with dx as float32 high and low parts as walk_jvp_ref.FakeTickJvp writes them."""

    def __init__(self, fake, nx, dpl, dplr, plant_nan=True):
        self.k, self.nx, self.dpl, self.dplr, self.plant_nan = fake, nx, dpl, dplr, plant_nan
        self.w = 9 + 6 * fake.M
        assert 2 * self.w <= nx

    def __call__(self, i, t, dl, dlr, ok):
        B, K = t.shape[:2]
        k = self.k
        v = np.concatenate([t, dl.reshape(B, K, -1)], 2)
        hi = v.astype(np.float32)
        x = np.zeros((B, K, self.nx), np.float32)
        x[:, :, :self.w], x[:, :, self.w:2 * self.w] = hi, (v - hi.astype(np.float64)).astype(np.float32)
        out = dict(state=k.f.a[i][:, None] * t + k.q[i][:, None] * dlr.reshape(B, K, -1)[:, :, :9], list=k.f.l[i][:, None] * dl + k.p[i][:, None] * self.dpl,
                   list_rot=k.lr[i][:, None] * dlr + k.pr[i][:, None] * self.dplr, x=x, sens=k.f.sens[i].copy())
        if self.plant_nan:
            for val in out.values():
                val[ok == 0] = np.nan
        return out

    def x64(self, x):
        return x[..., :self.w].astype(np.float64) + x[..., self.w:2 * self.w].astype(np.float64)
