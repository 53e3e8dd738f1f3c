"""numpy restatement of the forward walk's rule for ended problems (include/cmpc.h, cmpc_rollout_walk_jvp_device; DESIGN.md 7f, "Forwards") and a made-up
linear tick JVP to drive it with -- the transpose of tests/walk_tape_ref.py, coefficient for coefficient.  For problem b let e = end_tick[b], -1 read as
never; tick i is a good tick when e < 0 or i < e; t_i is the direction of the state tick i starts from, l_i that of the lists:

    t_{i+1} = [i < e] (the tick's state direction),    l_{i+1} = [i < e] (the tick's list directions),
    row i of dX = [i < e] (the tick's),    status_i = 6 and removed_i = 0 for i >= e,

and for i >= e the tick is fed ok = 0.  What enters a call behind a problem's end (e < tick0) is zero.  Everything is a selection (np.where), never a
product with a mask: what the tick leaves for an ended problem may be NaN, and so may its rows of what enters."""
import numpy as np

from tests.walk_tape_ref import SENS, ended


def _sel(en, a, zero=0.0):
    """zero where the problem has ended; en[B] against a[B, ...]"""
    return np.where(en.reshape((-1,) + (1,) * (a.ndim - 1)), a.dtype.type(zero), a)


def gate_pre(e, tick_pre, ok_row, first, state=None, lst=None, lst_rot=None):
    """-> ok_out, and with `first` the directions that enter the call, zero where e < tick_pre"""
    ok_out = np.where(ended(e, tick_pre), 0, ok_row if ok_row is not None else 1).astype(np.int32)
    if not first:
        return ok_out, state, lst, lst_rot
    gone = ended(e, tick_pre - 1)
    return (ok_out,) + tuple(None if a is None else _sel(gone, a) for a in (state, lst, lst_rot))


def gate_post(e, tick_post, o):
    """what the tick left (dict: state, list, list_rot, x -- the last two may be None -- and sens) -> the same keys gated, plus status and removed"""
    en = ended(e, tick_post)
    out = {k: None if o.get(k) is None else _sel(en, o[k]) for k in ("state", "list", "list_rot", "x")}
    out["status"] = np.where(en, 6, np.where(en, np.float32(0), o["sens"][:, 0]).astype(np.int32)).astype(np.int32)
    out["removed"] = np.where(en, np.float32(0), o["sens"][:, 6]).astype(np.float32)
    return out


class FakeTickJvp:
    """The transpose of walk_tape_ref.FakeTick, built on that object's coefficients a and l, elementwise so that float64 results do not depend on a
    summation order.  FakeTick is  state = a_i * carry_state + gx[:, :9],  list = l_i * carry_list + gx[:, 9:9 + 6 M];  its transpose is
        state' = a_i * t,   list' = l_i * dl,   dx[:9] = t,   dx[9:9 + 6 M] = dl,
    and the orientation directions get list_rot' = l_i * dlr of their own.  dx is float32 in the interface, so t and dl are written as float32 pairs:
    the high parts at [0, 9 + 6 M) and the low parts (v - float64(float32(v)), rounded) behind them at [9 + 6 M, 2 (9 + 6 M)); x64() puts them together.
    Word 0 and word 6 of sens are FakeTick's.  plant_nan: a problem fed ok = 0 gets NaN in every output -- the gate must select them away."""

    def __init__(self, fake, nx, plant_nan=True):
        self.f, self.nx, self.plant_nan = fake, nx, plant_nan
        self.w = 9 + 6 * fake.M
        assert 2 * self.w <= nx

    def __call__(self, i, t, dl, dlr, ok):
        B, K = t.shape[:2]
        a, l = self.f.a[i][:, None], self.f.l[i][:, None]
        v = np.concatenate([t, dl.reshape(B, K, -1)], 2)
        hi = v.astype(np.float32)
        x = np.zeros((B, K, self.nx), np.float32)
        x[:, :, :self.w], x[:, :, self.w:2 * self.w] = hi, (v - hi.astype(np.float64)).astype(np.float32)
        out = dict(state=a * t, list=l * dl, list_rot=None if dlr is None else l * dlr, x=x, sens=self.f.sens[i].copy())
        if self.plant_nan:
            for val in out.values():
                if val is not None:
                    val[ok == 0] = np.nan
        return out

    def x64(self, x):
        """[.., nx] float32 pairs -> [.., 9 + 6 M] float64"""
        return x[..., :self.w].astype(np.float64) + x[..., self.w:2 * self.w].astype(np.float64)


def forward_walk(tick, e, tick0, ticks, row0, ok, state_in, list_in, list_rot_in=None):
    """rows row0 .. row0 + ticks - 1 forwards under the rule; tick = a FakeTickJvp.  -> dict(states: the rows row0 .. row0 + ticks by row (row0: what
    entered, gated); list, list_rot: the directions leaving the last row; x, status, removed: the rows written, by row; fed: the ok words each tick got)"""
    ok0, t, dl, dlr = gate_pre(e, tick0, ok[row0], True, state_in, list_in, list_rot_in)
    out = dict(states={row0: t}, x={}, status={}, removed={}, fed={})
    for i in range(ticks):
        tk, r = tick0 + i, row0 + i
        f_ok = ok0 if i == 0 else gate_pre(e, tk, ok[r], False)[0]
        out["fed"][r] = f_ok
        g = gate_post(e, tk, tick(r, t, dl, dlr, f_ok))
        t, dl, dlr = g["state"], g["list"], g["list_rot"]
        out["states"][r + 1], out["x"][r], out["status"][r], out["removed"][r] = t, g["x"], g["status"], g["removed"]
    out["list"], out["list_rot"] = dl, dlr
    return out
