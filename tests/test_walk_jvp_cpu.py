"""The forward walk's rule for ended problems on the CPU: the host gate cmpc_rollout_walk_jvp_gate (no GPU, no solve) driven over a made-up linear tick JVP
(tests/walk_jvp_ref.py) against the numpy restatement -- problems that never end, end at tick 0, "at tick T" (behind the walk) and in the middle; a walk
in two segments through the carries; NaN planted in everything the tick leaves for an ended problem and in its rows of what enters; the rule as the exact
transpose of the reverse rule of tests/walk_tape_ref.py -- and the argument checks of the new entry points that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import cmpc_amd as cm
from tests import walk_jvp_ref as wj
from tests import walk_tape_ref as wt

N, M, T, K = 10, 3, 6, 3
END = np.concatenate([[-1, 0, T], np.random.default_rng(1).integers(1, T, 4)]).astype(np.int32)      # never, at once, behind the walk, and four in the middle
B = len(END)
NX = cm.Layout(N).nx


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _gate(e, Bn=B, k=K, **kw):
    g = cm._capi.CmpcWalkJvpGate()
    g.batch, g.max_contacts, g.horizon, g.k, g.end_tick = Bn, M, N, k, _ptr(e)
    for name, v in kw.items():
        setattr(g, name, v)
    return g


def host_forward_walk(lib, tick, e, tick0, ticks, row0, ok, state_in, list_in, list_rot_in=None):
    """the loop of cmpc_rollout_walk_jvp_device on the host: gate (PRE), tick, gate (POST + PRE), ..., gate (POST), the tick being `tick`"""
    Bn, k = state_in.shape[:2]
    t, dl = state_in.copy(), list_in.copy()
    dlr = None if list_rot_in is None else list_rot_in.copy()
    ok_out = np.full((Bn,), -9, np.int32)
    out = dict(states={}, x={}, status={}, removed={}, fed={})
    o = None
    for i in range(ticks + 1):
        g = _gate(e, Bn, k, do_post=int(i > 0), tick_post=tick0 + i - 1, do_pre=int(i < ticks), tick_pre=tick0 + i, first=int(i == 0))
        if i > 0:
            status, removed = np.full((Bn,), -9, np.int32), np.full((Bn,), -9.0, np.float32)
            g.tick_sens, g.state_out, g.list_out, g.list_rot_out, g.x_row = _ptr(o["sens"]), _ptr(o["state"]), _ptr(o["list"]), _ptr(o["list_rot"]), _ptr(o["x"])
            g.status_row, g.removed_row = _ptr(status), _ptr(removed)
        if i < ticks:
            g.ok_row, g.ok_out = _ptr(ok[row0 + i]), _ptr(ok_out)
            if i == 0:
                g.first_state, g.first_list, g.first_list_rot = _ptr(t), _ptr(dl), _ptr(dlr)
        assert lib.cmpc_rollout_walk_jvp_gate(C.byref(g)) == 0
        if i == 0:
            out["states"][row0] = t.copy()
        else:
            r = row0 + i - 1
            t, dl, dlr = o["state"], o["list"], o["list_rot"]
            out["states"][r + 1], out["x"][r], out["status"][r], out["removed"][r] = t, o["x"], status, removed
        if i == ticks:
            break
        out["fed"][row0 + i] = ok_out.copy()
        o = tick(row0 + i, t.copy(), dl.copy(), None if dlr is None else dlr.copy(), ok_out.copy())
    out["list"], out["list_rot"] = dl, dlr
    return out


def _case(seed, plant_nan=True):
    rng = np.random.default_rng(seed)
    L = cm.Layout(N)
    fake = wt.FakeTick(T, B, M, N, L.nx, L.np, seed + 1)
    fake.sens[:, :, 6] = rng.uniform(0.0, 1.0, (T, B)).astype(np.float32)
    tick = wj.FakeTickJvp(fake, L.nx, plant_nan)
    ok = np.ones((T, B), np.int32)      # (the made-up tick answers ok = 0 with NaN: only the gate may feed it one)
    return tick, ok, rng.normal(size=(B, K, 9)), rng.normal(size=(B, K, 2, M, 3)), rng.normal(size=(B, K, 2, M, 3))


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    for k in ("list", "list_rot"):
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            np.testing.assert_array_equal(_u(a[k]), _u(b[k]), err_msg=k)
    for k in ("states", "x", "status", "removed"):
        assert sorted(a[k]) == sorted(b[k]), k
        for r in a[k]:
            np.testing.assert_array_equal(_u(a[k][r]), _u(b[k][r]), err_msg=f"{k} row {r}")


def test_end_ticks_cover_the_cases():
    assert (END == -1).any() and (END == 0).any() and (END == T).any() and ((END > 0) & (END < T)).any()


@pytest.mark.parametrize("kind,t_post,with_x,with_rot", [("pre", -1, True, True), ("pre", 3, True, False), ("both", 0, True, True), ("both", 3, False, True),
                                                         ("both", 2, True, False), ("post", T - 1, True, True)])
def test_host_gate_step_matches_the_restatement(kind, t_post, with_x, with_rot):
    """one gate step of each kind, NaN in everything the tick left for an ended problem and in its rows of what enters: every array to the bit, every
    output finite, ended rows exactly zero with status 6 and removed 0"""
    lib = cm._capi.lib()
    rng = np.random.default_rng(11 + t_post)
    e = END
    t_pre = t_post + 1
    o = dict(state=rng.normal(size=(B, K, 9)), list=rng.normal(size=(B, K, 2, M, 3)), list_rot=rng.normal(size=(B, K, 2, M, 3)) if with_rot else None,
             x=rng.normal(size=(B, K, NX)).astype(np.float32) if with_x else None, sens=rng.integers(0, 6, (B, wt.SENS)).astype(np.float32))
    first = dict(state=rng.normal(size=(B, K, 9)), list=rng.normal(size=(B, K, 2, M, 3)), list_rot=rng.normal(size=(B, K, 2, M, 3)) if with_rot else None)
    ok_row = rng.integers(0, 2, B).astype(np.int32)
    if kind != "pre":
        for v in o.values():
            if v is not None:
                v[wt.ended(e, t_post)] = np.nan
    else:
        for v in first.values():
            if v is not None:
                v[wt.ended(e, t_pre - 1)] = np.nan
    want_post = wj.gate_post(e, t_post, o) if kind != "pre" else None
    want_pre = wj.gate_pre(e, t_pre, ok_row, kind == "pre", first["state"], first["list"], first["list_rot"]) if kind != "post" else None
    status, removed, ok_out = np.full((B,), -9, np.int32), np.full((B,), -9.0, np.float32), np.full((B,), -9, np.int32)
    g = _gate(e, do_post=int(kind != "pre"), tick_post=t_post, do_pre=int(kind != "post"), tick_pre=t_pre, first=int(kind == "pre"),
              tick_sens=_ptr(o["sens"]), state_out=_ptr(o["state"]), list_out=_ptr(o["list"]), list_rot_out=_ptr(o["list_rot"]), x_row=_ptr(o["x"]),
              status_row=_ptr(status), removed_row=_ptr(removed), ok_row=_ptr(ok_row), ok_out=_ptr(ok_out), first_state=_ptr(first["state"]),
              first_list=_ptr(first["list"]), first_list_rot=_ptr(first["list_rot"]))
    assert lib.cmpc_rollout_walk_jvp_gate(C.byref(g)) == 0
    if kind != "pre":
        en = wt.ended(e, t_post)
        for k in ("state", "list", "list_rot", "x"):
            if o[k] is not None:
                np.testing.assert_array_equal(_u(o[k]), _u(want_post[k]), err_msg=k)
                assert np.isfinite(o[k]).all() and (o[k][en] == 0).all(), k
        np.testing.assert_array_equal(status, want_post["status"])
        np.testing.assert_array_equal(_u(removed), _u(want_post["removed"]))
        assert (status[en] == 6).all() and (removed[en] == 0).all() and (status[~en] == o["sens"][~en, 0]).all() and (removed[~en] == o["sens"][~en, 6]).all()
    else:
        assert (status == -9).all() and (removed == -9.0).all()
    if kind != "post":
        np.testing.assert_array_equal(ok_out, want_pre[0])
        assert (ok_out[wt.ended(e, t_pre)] == 0).all() and (ok_out[~wt.ended(e, t_pre)] == ok_row[~wt.ended(e, t_pre)]).all()
    else:
        assert (ok_out == -9).all()
    if kind == "pre":
        for k, w in zip(("state", "list", "list_rot"), want_pre[1:]):
            if first[k] is not None:
                np.testing.assert_array_equal(_u(first[k]), _u(w), err_msg=k)
                assert np.isfinite(first[k]).all()


@pytest.mark.parametrize("with_rot", [True, False])
def test_host_loop_matches_the_restatement(with_rot):
    lib = cm._capi.lib()
    tick, ok, t0, l0, lr0 = _case(3)
    lr0 = lr0 if with_rot else None
    got = host_forward_walk(lib, tick, END, 0, T, 0, ok, t0, l0, lr0)
    want = wj.forward_walk(tick, END, 0, T, 0, ok, t0, l0, lr0)
    _same(got, want)
    for r in range(T):
        np.testing.assert_array_equal(got["fed"][r], want["fed"][r], err_msg=f"fed, row {r}")
        en = wt.ended(END, r)
        assert (got["fed"][r][en] == 0).all() and (got["status"][r][en] == 6).all() and (got["removed"][r][en] == 0).all()
        assert (got["x"][r][en] == 0).all() and (got["states"][r + 1][en] == 0).all()
        assert (got["status"][r][~en] == tick.f.sens[r, ~en, 0].astype(np.int32)).all()
        assert np.isfinite(got["x"][r]).all() and np.isfinite(got["states"][r + 1]).all()
    assert np.isfinite(got["list"]).all() and (got["list"][END >= 0][END[END >= 0] < T] == 0).all()
    # the rule against the recursion written out: t_i = a_{i-1} ... a_0 t_0 while i <= e, zero behind
    for b, e in enumerate(END):
        last = T if e < 0 else min(int(e), T)
        v = t0[b].copy()
        for i in range(T + 1):
            np.testing.assert_array_equal(got["states"][i][b], v if i <= last else np.zeros_like(v), err_msg=f"problem {b}, state {i}")
            if i < T:
                v = tick.f.a[i, b][None] * v
    np.testing.assert_array_equal(got["states"][0][1], t0[1])      # e = 0: t_0 is the caller's, everything behind it zero
    assert (got["states"][1][1] == 0).all()


@pytest.mark.parametrize("cut", [1, 3, 5])
def test_segments_compose_through_the_carries(cut):
    """rows 0 .. cut - 1 and then cut .. T - 1 through the state row and the list carries against one pass over 0 .. T - 1: every bit; NaN handed to the
    second segment in the rows of a problem that ended before it is selected away"""
    lib = cm._capi.lib()
    tick, ok, t0, l0, lr0 = _case(5)
    one = host_forward_walk(lib, tick, END, 0, T, 0, ok, t0, l0, lr0)
    lo = host_forward_walk(lib, tick, END, 0, cut, 0, ok, t0, l0, lr0)
    hi = host_forward_walk(lib, tick, END, cut, T - cut, cut, ok, lo["states"][cut], lo["list"], lo["list_rot"])
    two = dict(list=hi["list"], list_rot=hi["list_rot"], **{k: {**lo[k], **hi[k]} for k in ("states", "x", "status", "removed")})
    _same(one, two)
    gone = wt.ended(END, cut - 1)
    assert gone.any()
    bad = [a.copy() for a in (lo["states"][cut], lo["list"], lo["list_rot"])]
    for a in bad:
        a[gone] = np.nan
    hi2 = host_forward_walk(lib, tick, END, cut, T - cut, cut, ok, *bad)
    _same(hi, hi2)
    _same(hi, wj.forward_walk(tick, END, cut, T - cut, cut, ok, *bad))


def test_the_rule_is_the_transpose_of_the_reverse_rule():
    """with the same coefficients, walk_tape_ref.reverse_walk (seeds G on the states, GX on the solutions) and the forward walk through the host gate satisfy
    sum_i <G_i, t_i> + sum_i <GX_i, dX_i> = <c_0, t_0> + <list carry_0, l_0> per problem and column, ended problems included: the forward zeros behind an end
    meet the seeds the reverse rule does not read.  Bound 1e-12 relative to the larger side: float64 elementwise products on both sides, the float32
    solution direction carried as high and low parts (walk_jvp_ref.FakeTickJvp)."""
    lib = cm._capi.lib()
    rng = np.random.default_rng(9)
    L = cm.Layout(N)
    fake = wt.FakeTick(T, B, M, N, L.nx, L.np, 10)
    tick = wj.FakeTickJvp(fake, L.nx)
    ok = np.ones((T, B), np.int32)
    t0, l0 = rng.normal(size=(B, K, 9)), rng.normal(size=(B, K, 2, M, 3))
    G = rng.normal(size=(T + 1, B, 9))
    GX = np.zeros((T, B, L.nx), np.float32)
    GX[:, :, :tick.w] = rng.normal(size=(T, B, tick.w)).astype(np.float32)
    fwd = host_forward_walk(lib, tick, END, 0, T, 0, ok, t0, l0)
    rev = wt.reverse_walk(fake, END, 0, T, 0, G, GX, ok, G[T].copy(), np.zeros((B, 2, M, 3)))
    worst, ended_nonzero = 0.0, 0
    for b in range(B):
        for j in range(K):
            lhs = sum(float((G[i, b] * fwd["states"][i][b, j]).sum()) for i in range(T + 1))
            lhs += sum(float((GX[i, b, :tick.w].astype(np.float64) * tick.x64(fwd["x"][i][b, j])).sum()) for i in range(T))
            rhs = float((rev["state"][b] * t0[b, j]).sum() + (rev["list"][b] * l0[b, j]).sum())
            worst = max(worst, abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300))
            ended_nonzero += int(0 <= END[b] < T and lhs != 0.0)
    print(f"\nforward rule against reverse rule, worst relative gap over {B} problems x {K} columns: {worst:.2e} (bound 1e-12)")
    assert worst <= 1e-12 and ended_nonzero > 0


def test_argument_checks_without_a_gpu():
    lib = cm._capi.lib()
    tape, d = cm._capi.CmpcWalkTape(), cm._capi.CmpcWalkDirs()
    # the walk: a NULL handle, k = 0, rows outside the tape, missing required pointers -- each refused before anything touches a GPU
    assert lib.cmpc_rollout_walk_jvp_device(None, M, 0, 1, C.byref(tape), 0, None, 1, C.byref(d), None) != 0
    assert lib.cmpc_rollout_walk_jvp_device(None, M, 0, 1, C.byref(tape), 0, None, 0, C.byref(d), None) != 0
    assert lib.cmpc_rollout_walk_jvp_device(None, M, 0, 2, C.byref(tape), 5, None, 1, C.byref(d), None) != 0
    assert lib.cmpc_rollout_walk_jvp_device(None, M, 0, 1, None, 0, None, 1, None, None) != 0
    assert lib.cmpc_rollout_walk_jvp_gate_device(None, C.byref(cm._capi.CmpcWalkJvpGate()), None) != 0
    # the host gate
    okb, st, ls, sens, status = np.zeros((B,), np.int32), np.zeros((B, K, 9)), np.zeros((B, K, 2, M, 3)), np.zeros((B, wt.SENS), np.float32), np.zeros((B,), np.int32)

    def gate(**kw):
        g = _gate(None, do_pre=1, tick_pre=0, ok_out=_ptr(okb))
        for k, v in kw.items():
            setattr(g, k, v)
        return lib.cmpc_rollout_walk_jvp_gate(C.byref(g))
    post = dict(do_post=1, tick_sens=_ptr(sens), state_out=_ptr(st), list_out=_ptr(ls), status_row=_ptr(status))
    assert gate() == 0 and gate(**post) == 0
    assert gate(batch=0) != 0 and gate(max_contacts=0) != 0 and gate(horizon=0) != 0 and gate(k=0) != 0 and gate(ok_out=None) != 0
    assert gate(do_pre=0) != 0                               # neither part
    assert gate(do_post=1) != 0                              # the POST part without its arrays
    for missing in ("tick_sens", "state_out", "list_out", "status_row"):
        assert gate(**{**post, missing: None}) != 0, missing
    assert lib.cmpc_rollout_walk_jvp_gate(None) != 0


def test_exports_and_struct_sizes():
    lib = cm._capi.lib()
    for name in ("cmpc_rollout_walk_jvp_device", "cmpc_rollout_walk_jvp_gate", "cmpc_rollout_walk_jvp_gate_device"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name), name
    # the ctypes mirrors have the C structs' sizes (LP64: pointers 8, ints 4, padded to 8)
    assert C.sizeof(cm._capi.CmpcWalkDirs) == 11 * 8
    assert C.sizeof(cm._capi.CmpcWalkJvpGate) == 16 + 8 + 8 + 7 * 8 + 16 + 5 * 8
    # the pinned layouts next to them are untouched
    assert C.sizeof(cm._capi.CmpcWalkGrads) == 9 * 8 and C.sizeof(cm._capi.CmpcWalkGate) == 16 + 8 + 8 + 9 * 8 + 16 + 4 * 8


def test_python_surface_of_the_forward_walk():
    import inspect
    ro = cm.rollout.WalkingRollout
    assert list(inspect.signature(ro.forward_sensitivity_device).parameters) == [
        "self", "w", "dir_state0", "dir_list0", "dir_list_rot0", "dir_plan", "dir_plan_rot", "dir_push", "dir_models", "dir_wrench", "solutions"]
    assert list(inspect.signature(ro.forward_sensitivity_device).parameters)[2:] == list(inspect.signature(ro.forward_sensitivity).parameters)[2:]
    assert list(inspect.signature(ro.backward_device).parameters) == ["self", "w", "grad_states", "grad_X"]
    for name in ("rollout_walk_jvp_device", "rollout_walk_jvp_gate_device"):
        assert hasattr(cm.BatchSolver, name), name
    with pytest.raises(NotImplementedError):      # the orientation chain of the reverse device walk is still not built
        cm.rollout_differentiable(None, 1, None, plan_yaw=object(), device_walk=True)
    assert "no forward mode" not in cm.rollout_differentiable.__doc__ and "forward_sensitivity_device" in cm.rollout_differentiable.__doc__
