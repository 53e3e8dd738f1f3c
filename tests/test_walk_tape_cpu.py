"""The reverse walk's rule for ended problems on the CPU: the host gate cmpc_rollout_walk_vjp_gate (no GPU, no solve) driven over a made-up tick VJP
(tests/walk_tape_ref.py) against the numpy restatement -- problems that never end, end at tick 0, at the last tick, "at tick T" (behind the walk) and in
the middle; a walk reversed in two segments through the carries; NaN planted in everything the tick leaves for an ended problem and in the seeds behind
its end -- and the argument checks of the new entry points that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_tape_ref as wt

N, M, T = 10, 5, 6
END = np.array([-1, 0, T - 1, T, 2, 3, -1], np.int32)
B = len(END)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_reverse_walk(lib, tick, e, tick0, ticks, row0, G, GX, ok, carry_state, carry_list, N=N, M=M):
    """the loop of cmpc_rollout_walk_vjp_device on the host: gate (PRE), tick, gate (POST + PRE), ..., gate (POST), the tick being `tick`"""
    L = cm.Layout(N)
    Bn = G.shape[1]
    c, cl = carry_state.copy(), carry_list.copy()
    ok_out = np.full((Bn,), -9, np.int32)
    gx_out = np.full((Bn, L.nx), 7.0, np.float32) if GX is not None else None
    out = dict(wrench={}, gp={}, status={}, fed={})
    o = None
    for i in range(ticks, -1, -1):
        g = cm._capi.CmpcWalkGate()
        g.batch, g.max_contacts, g.horizon, g.end_tick = Bn, M, N, _ptr(e)
        g.carry_state, g.carry_list = _ptr(c), _ptr(cl)
        g.do_post, g.tick_post = int(i < ticks), tick0 + i
        if i < ticks:
            r = row0 + i
            status = np.full((Bn,), -9, np.int32)
            g.seed_state, g.tick_state, g.tick_list, g.tick_sens = _ptr(G[r]), _ptr(o["state"]), _ptr(o["list"]), _ptr(o["sens"])
            g.wrench_row, g.grad_p_row, g.status_row = _ptr(o["wrench"]), _ptr(o["gp"]), _ptr(status)
        g.do_pre, g.tick_pre, g.first = int(i > 0), tick0 + i - 1, int(i == ticks)
        if i > 0:
            g.ok_row, g.ok_out = _ptr(ok[row0 + i - 1]), _ptr(ok_out)
            if GX is not None:
                g.grad_x_row, g.grad_x_out = _ptr(GX[row0 + i - 1]), _ptr(gx_out)
        assert lib.cmpc_rollout_walk_vjp_gate(C.byref(g)) == 0
        if i < ticks:
            out["wrench"][r], out["gp"][r], out["status"][r] = o["wrench"], o["gp"], status
        if i == 0:
            break
        r = row0 + i - 1
        out["fed"][r] = (c.copy(), cl.copy(), None if GX is None else gx_out.copy(), ok_out.copy())
        o = tick(r, c.copy(), cl.copy(), None if GX is None else gx_out.copy(), ok_out.copy())
    out["state"], out["list"] = c, cl
    return out


def _case(seed, with_gx=True, nan_seeds=True):
    rng = np.random.default_rng(seed)
    L = cm.Layout(N)
    G = rng.normal(size=(T + 1, B, 9))
    GX = rng.normal(size=(T, B, L.nx)).astype(np.float32) if with_gx else None
    if nan_seeds:      # the seeds behind a problem's end are not read
        for b, e in enumerate(END):
            if 0 <= e < T:
                G[e + 1:, b] = np.nan
                if GX is not None:
                    GX[e:, b] = np.nan
    ok = np.ones((T, B), np.int32)
    tick = wt.FakeTick(T, B, M, N, L.nx, L.np, seed + 1)
    return tick, G, GX, ok


def _same(a, b):
    for k in ("state", "list"):
        np.testing.assert_array_equal(a[k].view(np.uint64), b[k].view(np.uint64), err_msg=k)
    for k in ("wrench", "gp", "status"):
        assert sorted(a[k]) == sorted(b[k])
        for r in a[k]:
            x, y = np.ascontiguousarray(a[k][r]), np.ascontiguousarray(b[k][r])
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{k} row {r}")


@pytest.mark.parametrize("with_gx", [True, False])
def test_host_gate_matches_the_restatement(with_gx):
    lib = cm._capi.lib()
    tick, G, GX, ok = _case(3, with_gx)
    c0, l0 = G[T].copy(), np.zeros((B, 2, M, 3))
    got = host_reverse_walk(lib, tick, END, 0, T, 0, G, GX, ok, c0, l0)
    want = wt.reverse_walk(tick, END, 0, T, 0, G, GX, ok, c0, l0)
    _same(got, want)
    for r in range(T):      # what the tick was fed: zeros and ok = 0 behind the end, the carries and seeds themselves elsewhere
        for x, y in zip(got["fed"][r], want["fed"][r]):
            if x is not None:
                np.testing.assert_array_equal(x, y, err_msg=f"fed, row {r}")
    # no NaN anywhere although the tick's outputs and the seeds of ended problems were NaN; ended rows are exact zeros with status 6
    for k in ("state", "list"):
        assert np.isfinite(got[k]).all(), k
    for r in range(T):
        en = wt.ended(END, r)
        assert np.isfinite(got["wrench"][r]).all() and np.isfinite(got["gp"][r]).all()
        assert (got["wrench"][r][en] == 0).all() and (got["gp"][r][en] == 0).all() and (got["status"][r][en] == 6).all()
        assert (got["status"][r][~en] == tick.sens[r, ~en, 0].astype(np.int32)).all()
    # the carry rule against the loss itself: e = 0 leaves exactly G_0, e = T is a problem that walked to the end
    np.testing.assert_array_equal(got["state"][1], G[0, 1])
    assert (got["list"][1] == 0).all()
    Gz, GXz = np.nan_to_num(G), None if GX is None else np.nan_to_num(GX)
    np.testing.assert_allclose(got["state"], wt.closed_form_state0(tick, END, T, Gz, GXz), rtol=1e-12, atol=1e-12)
    whole = wt.closed_form_state0(tick, np.full((B,), -1, np.int32), T, Gz, GXz)
    np.testing.assert_allclose(got["state"][[0, 3, 6]], whole[[0, 3, 6]], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cut", [1, 3, 5])
def test_segments_compose_through_the_carries(cut):
    """rows cut .. T - 1 and then 0 .. cut - 1 through the carry buffers against one pass over 0 .. T - 1: every bit.  cut = 3 is the tick problem 5 ends
    at, cut = 1 lies behind the end of problem 1, cut = 5 is the last tick (problem 2's end)"""
    lib = cm._capi.lib()
    tick, G, GX, ok = _case(5)
    c0, l0 = G[T].copy(), np.zeros((B, 2, M, 3))
    one = host_reverse_walk(lib, tick, END, 0, T, 0, G, GX, ok, c0, l0)
    hi = host_reverse_walk(lib, tick, END, cut, T - cut, cut, G, GX, ok, c0, l0)
    lo = host_reverse_walk(lib, tick, END, 0, cut, 0, G, GX, ok, hi["state"], hi["list"])
    two = dict(state=lo["state"], list=lo["list"], **{k: {**hi[k], **lo[k]} for k in ("wrench", "gp", "status")})
    _same(one, two)
    # a garbage carry handed to a segment whose last tick lies behind a problem's end is selected away
    bad_c, bad_l = hi["state"].copy(), hi["list"].copy()
    en = wt.ended(END, cut - 1)
    bad_c[en], bad_l[en] = np.nan, np.nan
    lo2 = host_reverse_walk(lib, tick, END, 0, cut, 0, G, GX, ok, bad_c, bad_l)
    _same(lo, lo2)


def test_host_gate_without_an_end_mask_and_bad_arguments():
    lib = cm._capi.lib()
    tick, G, GX, ok = _case(7, nan_seeds=False)
    tick.plant_nan = False
    c0, l0 = G[T].copy(), np.zeros((B, 2, M, 3))
    never = np.full((B,), -1, np.int32)
    _same(host_reverse_walk(lib, tick, None, 0, T, 0, G, GX, ok, c0, l0), wt.reverse_walk(tick, never, 0, T, 0, G, GX, ok, c0, l0))
    L = cm.Layout(N)
    c, cl = np.zeros((B, 9)), np.zeros((B, 2, M, 3))
    okb, gxb = np.zeros((B,), np.int32), np.zeros((B, L.nx), np.float32)

    def gate(**kw):
        g = cm._capi.CmpcWalkGate()
        g.batch, g.max_contacts, g.horizon, g.carry_state, g.carry_list = B, M, N, _ptr(c), _ptr(cl)
        g.do_pre, g.tick_pre, g.ok_out = 1, 0, _ptr(okb)
        for k, v in kw.items():
            setattr(g, k, v)
        return lib.cmpc_rollout_walk_vjp_gate(C.byref(g))
    assert gate() == 0
    assert gate(batch=0) != 0 and gate(max_contacts=0) != 0 and gate(horizon=0) != 0 and gate(carry_state=None) != 0 and gate(ok_out=None) != 0
    assert gate(do_pre=0) != 0                               # neither part
    assert gate(do_post=1) != 0                              # the POST part without its arrays
    assert gate(grad_x_row=_ptr(gxb)) != 0                   # seeds on x without the gated copy's buffer
    assert lib.cmpc_rollout_walk_vjp_gate(None) != 0


def test_new_entry_points_check_their_arguments_without_a_gpu():
    lib = cm._capi.lib()
    tape, io, g = cm._capi.CmpcWalkTape(), cm._capi.CmpcWalkIO(), cm._capi.CmpcWalkGrads()
    assert lib.cmpc_rollout_tape_device(None, M, 0, 3, *([None] * 11), C.byref(tape), None) != 0
    assert lib.cmpc_rollout_walk_taped_device(None, M, 0, 1, 1, C.byref(io), None, 0, 0, None, C.byref(tape), 0, None) != 0
    assert lib.cmpc_rollout_walk_vjp_device(None, M, 0, 1, C.byref(tape), 0, None, C.byref(g), None) != 0
    for name in ("cmpc_rollout_tape_device", "cmpc_rollout_walk_taped_device", "cmpc_rollout_walk_vjp_device", "cmpc_rollout_walk_vjp_gate"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name), name
    # the ctypes mirrors have the C structs' sizes (LP64: pointers and doubles 8, ints 4, padded to 8)
    assert C.sizeof(cm._capi.CmpcWalkTape) == 8 + 11 * 8 + 8 + 3 * 4 + 4
    assert C.sizeof(cm._capi.CmpcWalkGrads) == 9 * 8
    assert C.sizeof(cm._capi.CmpcWalkGate) == 16 + 8 + 8 + 9 * 8 + 16 + 4 * 8


def test_python_surface_of_the_taped_walk():
    import inspect
    ro = cm.rollout.WalkingRollout
    assert list(inspect.signature(ro.walk_device_taped).parameters)[:5] == ["self", "ticks", "com0", "dcom0", "h0"]
    assert list(inspect.signature(ro.backward_device).parameters) == ["self", "w", "grad_states", "grad_X"]
    p = inspect.signature(cm.rollout_differentiable).parameters
    assert p["device_walk"].default is False and p["replan"].default is None
    with pytest.raises(NotImplementedError):      # the orientation chain is not on the device tape: said before anything touches a GPU
        cm.rollout_differentiable(None, 1, None, plan_yaw=object(), device_walk=True)
    with pytest.raises(NotImplementedError):
        cm.rollout_differentiable(None, 1, None, replan={})
    for name in ("walk_tape", "rollout_tape_device", "rollout_walk_vjp_device", "rollout_walk_vjp_gate_device"):
        assert hasattr(cm.BatchSolver, name), name
    assert "tape" in inspect.signature(cm.BatchSolver.rollout_walk_device).parameters
