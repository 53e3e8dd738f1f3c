"""The reverse walk with the orientation chain on the CPU: the host gate cmpc_rollout_walk_vjp_rot_gate (no GPU, no solve) against the numpy restatement
(tests/walk_rot_tape_ref.py), its `base` outputs against cmpc_rollout_walk_vjp_gate to the bit, the host loops of the reverse and of the forward walk held
to each other as transposes over made-up linear ticks with ended problems, the right Jacobian of SO(3) and the plan rotation of rollout_differentiable, and
the argument checks of the new entry points that need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmpc_amd as cm
from tests import walk_rot_tape_ref as wr
from tests import walk_tape_ref as wt
from tests.test_walk_jvp_cpu import host_forward_walk      # (the forward loop through cmpc_rollout_walk_jvp_gate; it builds its gates for N = 10, M = 3)

rot_plan_poses, so3_right_jacobian, yaw_plan_poses = cm.rollout.rot_plan_poses, cm.rollout.so3_right_jacobian, cm.rollout.yaw_plan_poses

N, M, T, K = 10, 3, 6, 2
END = np.array([-1, 0, 3, -1, 2], np.int32)      # never, at tick 0, in the middle
B = len(END)
LAY = cm.Layout(N)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _base(e, Bn=B, **kw):
    g = cm._capi.CmpcWalkGate()
    g.batch, g.max_contacts, g.horizon, g.end_tick = Bn, M, N, _ptr(e)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _step_inputs(rng, e, kind, t_post):
    """the arrays of one gate step, NaN in every input row of the problems that have ended"""
    t_pre = t_post - 1
    a = dict(seed=rng.normal(size=(B, 9)), state=rng.normal(size=(B, 9)), list=rng.normal(size=(B, 2, M, 3)), list_rot=rng.normal(size=(B, 2, M, 3)),
             sens=rng.integers(0, 6, (B, wt.SENS)).astype(np.float32), wrench=rng.normal(size=(B, N, 6)).astype(np.float32),
             gp=rng.normal(size=(B, LAY.np)).astype(np.float32), rot=rng.normal(size=(B, 2, N, 3)), gx=rng.normal(size=(B, LAY.nx)).astype(np.float32),
             ok=rng.integers(0, 2, B).astype(np.int32), c=rng.normal(size=(B, 9)), cl=rng.normal(size=(B, 2, M, 3)), cr=rng.normal(size=(B, 2, M, 3)))
    if kind != "pre":
        en = wt.ended(e, t_post)
        for k in ("state", "list", "list_rot", "sens", "wrench", "gp", "rot"):
            a[k][en] = np.nan
        a["seed"][en & (e != t_post)] = np.nan      # (the seed on s_e is read: it is the carry)
    if kind != "post":
        en = wt.ended(e, t_pre)
        a["gx"][en] = np.nan
        if kind == "pre":
            for k in ("c", "cl", "cr"):
                a[k][en] = np.nan
    return a


def _run_step(lib, e, kind, t_post, a, rot=True):
    """one gate step through the C function on copies of a's arrays -> what it wrote"""
    a = {k: v.copy() for k, v in a.items()}
    out = dict(status=np.full((B,), -9, np.int32), removed=np.full((B,), -9.0, np.float32), ok_out=np.full((B,), -9, np.int32),
               gx_out=np.full((B, LAY.nx), 7.0, np.float32))
    base = _base(e, carry_state=_ptr(a["c"]), carry_list=_ptr(a["cl"]), do_post=int(kind != "pre"), tick_post=t_post, do_pre=int(kind != "post"),
                 tick_pre=t_post - 1, first=int(kind == "pre"))
    if kind != "pre":
        base.seed_state, base.tick_state, base.tick_list, base.tick_sens = _ptr(a["seed"]), _ptr(a["state"]), _ptr(a["list"]), _ptr(a["sens"])
        base.wrench_row, base.grad_p_row, base.status_row = _ptr(a["wrench"]), _ptr(a["gp"]), _ptr(out["status"])
    if kind != "post":
        base.ok_row, base.grad_x_row, base.ok_out, base.grad_x_out = _ptr(a["ok"]), _ptr(a["gx"]), _ptr(out["ok_out"]), _ptr(out["gx_out"])
    if rot:
        g = cm._capi.CmpcWalkGateRot()
        g.base = base
        g.tick_list_rot, g.carry_list_rot, g.rot_row, g.removed_row = _ptr(a["list_rot"]), _ptr(a["cr"]), _ptr(a["rot"]), _ptr(out["removed"])
        assert lib.cmpc_rollout_walk_vjp_rot_gate(C.byref(g)) == 0
    else:
        assert lib.cmpc_rollout_walk_vjp_gate(C.byref(base)) == 0
    out.update(c=a["c"], cl=a["cl"], cr=a["cr"], wrench=a["wrench"], gp=a["gp"], rot=a["rot"])
    return out


@pytest.mark.parametrize("kind,t_post", [("pre", 3), ("pre", T), ("post", 0), ("post", 4), ("both", 1), ("both", 3), ("both", 5)])
def test_host_gate_step_matches_the_restatement(kind, t_post):
    lib = cm._capi.lib()
    e = END
    a = _step_inputs(np.random.default_rng(20 + t_post), e, kind, t_post)
    got = _run_step(lib, e, kind, t_post, a)
    if kind != "pre":
        want = wr.gate_post(e, t_post, a["seed"], dict(state=a["state"], list=a["list"], list_rot=a["list_rot"], sens=a["sens"]),
                            dict(wrench=a["wrench"], gp=a["gp"], rot=a["rot"]))
        en = wt.ended(e, t_post)
        for k, w in (("c", "state"), ("cl", "list"), ("cr", "list_rot"), ("wrench", "wrench"), ("gp", "gp"), ("rot", "rot"), ("removed", "removed")):
            np.testing.assert_array_equal(_u(got[k]), _u(want[w]), err_msg=k)
            assert np.isfinite(got[k]).all(), k
            if k != "c":
                assert (got[k][en] == 0).all(), k
        np.testing.assert_array_equal(got["status"], want["status"])
        assert (got["status"][en] == 6).all() and (got["removed"][~en] == a["sens"][~en, 6]).all()
        # the state carry of an ended problem: exactly zero, or the seed on s_e
        for b in np.where(en)[0]:
            np.testing.assert_array_equal(got["c"][b], a["seed"][b] if e[b] == t_post else np.zeros(9))
        # a walking problem's row of dGradRot keeps the tick's bits
        np.testing.assert_array_equal(_u(got["rot"][~en]), _u(a["rot"][~en]))
    else:
        assert (got["status"] == -9).all() and (got["removed"] == -9.0).all()
    if kind != "post":
        ok_out, gx_out, c, cl, cr = wr.gate_pre(e, t_post - 1, a["ok"], a["gx"], kind == "pre", a["c"], a["cl"], a["cr"])
        np.testing.assert_array_equal(got["ok_out"], ok_out)
        np.testing.assert_array_equal(_u(got["gx_out"]), _u(gx_out))
        assert np.isfinite(got["gx_out"]).all() and (got["gx_out"][wt.ended(e, t_post - 1)] == 0).all()
        if kind == "pre":
            for k, w in (("c", c), ("cl", cl), ("cr", cr)):
                np.testing.assert_array_equal(_u(got[k]), _u(w), err_msg=k)
                assert np.isfinite(got[k]).all() and (got[k][wt.ended(e, t_post - 1)] == 0).all(), k
    else:
        assert (got["ok_out"] == -9).all()


def test_end_ticks_cover_the_cases():
    assert (END == -1).any() and (END == 0).any() and ((END > 0) & (END < T)).any()


@pytest.mark.parametrize("kind,t_post", [("pre", 3), ("post", 4), ("both", 3)])
def test_base_outputs_equal_the_gate_without_orientations(kind, t_post):
    """the same base driven through both functions: every base output to the bit"""
    lib = cm._capi.lib()
    a = _step_inputs(np.random.default_rng(40 + t_post), END, kind, t_post)
    with_rot, without = _run_step(lib, END, kind, t_post, a, rot=True), _run_step(lib, END, kind, t_post, a, rot=False)
    for k in ("c", "cl", "wrench", "gp", "status", "ok_out", "gx_out"):
        np.testing.assert_array_equal(_u(with_rot[k]), _u(without[k]), err_msg=k)
    np.testing.assert_array_equal(_u(without["cr"]), _u(a["cr"]))      # (and the plain gate knows nothing of the orientation arrays)
    np.testing.assert_array_equal(_u(without["rot"]), _u(a["rot"]))


def host_reverse_walk_rot(lib, tick, e, tick0, ticks, row0, G, GX, ok, c0, cl0, cr0, plan, plan_rot):
    """the loop of cmpc_rollout_walk_vjp_rot_device on the host: gate (PRE), tick, gate (POST + PRE), ..., gate (POST), the tick being `tick`; plan and
    plan_rot are added to in place"""
    Bn = G.shape[1]
    c, cl, cr = c0.copy(), cl0.copy(), cr0.copy()
    ok_out, gx_out = np.full((Bn,), -9, np.int32), np.full((Bn, LAY.nx), 7.0, np.float32)
    out = dict(rot={}, status={}, removed={})
    o = None
    for i in range(ticks, -1, -1):
        g = cm._capi.CmpcWalkGateRot()
        g.base = _base(e, Bn, carry_state=_ptr(c), carry_list=_ptr(cl), do_post=int(i < ticks), tick_post=tick0 + i, do_pre=int(i > 0), tick_pre=tick0 + i - 1,
                       first=int(i == ticks))
        g.carry_list_rot = _ptr(cr)
        if i < ticks:
            r = row0 + i
            status, removed = np.full((Bn,), -9, np.int32), np.full((Bn,), -9.0, np.float32)
            b = g.base
            b.seed_state, b.tick_state, b.tick_list, b.tick_sens = _ptr(G[r]), _ptr(o["state"]), _ptr(o["list"]), _ptr(o["sens"])
            b.wrench_row, b.grad_p_row, b.status_row = _ptr(o["wrench"]), _ptr(o["gp"]), _ptr(status)
            g.tick_list_rot, g.rot_row, g.removed_row = _ptr(o["list_rot"]), _ptr(o["rot"]), _ptr(removed)
        if i > 0:
            g.base.ok_row, g.base.ok_out = _ptr(ok[row0 + i - 1]), _ptr(ok_out)
            g.base.grad_x_row, g.base.grad_x_out = _ptr(GX[row0 + i - 1]), _ptr(gx_out)
        assert lib.cmpc_rollout_walk_vjp_rot_gate(C.byref(g)) == 0
        if i < ticks:
            out["rot"][r], out["status"][r], out["removed"][r] = o["rot"], status, removed
        if i == 0:
            break
        o = tick(row0 + i - 1, c.copy(), cl.copy(), cr.copy(), gx_out.copy(), ok_out.copy())
        plan += o["plan_add"]
        plan_rot += o["plan_rot_add"]
    out["state"], out["list"], out["list_rot"] = c, cl, cr
    return out


def _transpose_case(seed):
    rng = np.random.default_rng(seed)
    rev = wr.FakeTickRot(T, B, M, N, LAY.nx, LAY.np, seed + 1)
    dpl, dplr = rng.normal(size=(B, K, 2, M, 3)), rng.normal(size=(B, K, 2, M, 3))
    fwd = wr.FakeTickRotJvp(rev, LAY.nx, dpl, dplr)
    G = rng.normal(size=(T + 1, B, 9))
    GX = np.zeros((T, B, LAY.nx), np.float32)
    GX[:, :, :fwd.w] = rng.normal(size=(T, B, fwd.w)).astype(np.float32)
    for b, e in enumerate(END):      # the seeds behind a problem's end are not read
        if 0 <= e < T:
            G[e + 1:, b] = np.nan
            GX[e:, b] = np.nan
    return rng, rev, fwd, dpl, dplr, G, GX, np.ones((T, B), np.int32)


def test_the_reverse_walk_is_the_transpose_of_the_forward_walk():
    """sum_i <G_i, t_i> + <GX_i, dx_i> over all rows = <state0, t_0> + <list0, l_0> + <list_rot0, l_rot_0> + <plan, d plan> + <plan_rot, d plan_rot> per
    problem and column, ended problems included, both loops through the C gates.  Bound 1e-12 relative to the larger side, as tests/test_walk_jvp_cpu.py
    holds its identity: float64 elementwise products on both sides, the float32 solution direction carried as high and low parts."""
    lib = cm._capi.lib()
    rng, rev, fwd, dpl, dplr, G, GX, ok = _transpose_case(9)
    t0, l0, lr0 = rng.normal(size=(B, K, 9)), rng.normal(size=(B, K, 2, M, 3)), rng.normal(size=(B, K, 2, M, 3))
    f = host_forward_walk(lib, fwd, END, 0, T, 0, ok, t0, l0, lr0)
    plan, plan_rot = np.zeros((B, 2, M, 3)), np.zeros((B, 2, M, 3))
    r = host_reverse_walk_rot(lib, rev, END, 0, T, 0, G, GX, ok, G[T].copy(), np.zeros((B, 2, M, 3)), np.zeros((B, 2, M, 3)), plan, plan_rot)
    for k in ("state", "list", "list_rot"):
        assert np.isfinite(r[k]).all(), k
    assert np.isfinite(plan).all() and np.isfinite(plan_rot).all()
    Gz, GXz = np.nan_to_num(G), np.nan_to_num(GX)
    worst, ended_nonzero, rot_terms = 0.0, 0, 0
    for b in range(B):
        for j in range(K):
            lhs = sum(float((Gz[i, b] * f["states"][i][b, j]).sum()) for i in range(T + 1))
            lhs += sum(float((GXz[i, b, :fwd.w].astype(np.float64) * fwd.x64(f["x"][i][b, j])).sum()) for i in range(T))
            rot_part = float((r["list_rot"][b] * lr0[b, j]).sum() + (plan_rot[b] * dplr[b, j]).sum())
            rhs = float((r["state"][b] * t0[b, j]).sum() + (r["list"][b] * l0[b, j]).sum() + (plan[b] * dpl[b, j]).sum()) + rot_part
            worst = max(worst, abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300))
            ended_nonzero += int(0 <= END[b] < T and lhs != 0.0)
            rot_terms += int(rot_part != 0.0)
    print(f"\nreverse walk with orientations against the forward walk, worst relative gap over {B} problems x {K} columns: {worst:.2e} (bound 1e-12)")
    assert worst <= 1e-12 and ended_nonzero > 0 and rot_terms > 0
    # the rows of an ended problem: rot zero, removed 0, status 6; a problem that ended at tick 0 passes nothing but its seed
    for row in range(T):
        en = wt.ended(END, row)
        assert (r["rot"][row][en] == 0).all() and (r["removed"][row][en] == 0).all() and (r["status"][row][en] == 6).all()
        np.testing.assert_array_equal(_u(r["rot"][row][~en]), _u(rev.rot[row][~en]))
    np.testing.assert_array_equal(r["state"][1], G[0, 1])
    assert (r["list_rot"][1] == 0).all() and (plan_rot[1] == 0).all() and (plan[1] == 0).all()


def test_segments_compose_through_the_three_carries():
    lib = cm._capi.lib()
    _, rev, _, _, _, G, GX, ok = _transpose_case(13)
    z = lambda: np.zeros((B, 2, M, 3))
    p1, pr1, p2, pr2 = z(), z(), z(), z()
    one = host_reverse_walk_rot(lib, rev, END, 0, T, 0, G, GX, ok, G[T].copy(), z(), z(), p1, pr1)
    hi = host_reverse_walk_rot(lib, rev, END, 3, T - 3, 3, G, GX, ok, G[T].copy(), z(), z(), p2, pr2)
    lo = host_reverse_walk_rot(lib, rev, END, 0, 3, 0, G, GX, ok, hi["state"], hi["list"], hi["list_rot"], p2, pr2)
    for k in ("state", "list", "list_rot"):
        np.testing.assert_array_equal(_u(one[k]), _u(lo[k]), err_msg=k)
    np.testing.assert_array_equal(_u(p1), _u(p2))
    np.testing.assert_array_equal(_u(pr1), _u(pr2))
    for k in ("rot", "status", "removed"):
        two = {**hi[k], **lo[k]}
        for row in range(T):
            np.testing.assert_array_equal(_u(one[k][row]), _u(two[row]), err_msg=f"{k} row {row}")


# ---- the right Jacobian of SO(3) and the plan rotation ----
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _exp(w):
    t = np.linalg.norm(w)
    W = _hat(w)
    if t < 1e-7:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + np.sin(t) / t * W + (1.0 - np.cos(t)) / (t * t) * W @ W


def _log(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])      # sin(t) axis
    s = np.linalg.norm(v)
    return v if s < 1e-7 else v * (np.arcsin(s) / s)                                    # (rotations near the identity only)


@pytest.mark.parametrize("norm", [0.0, 1e-9, 0.2, 1.0])
def test_right_jacobian_against_central_differences(norm):
    """Jr(omega) e_i = d/dh Log(Exp(omega)^-1 Exp(omega + h e_i)) at h = 0, central differences at h = 1e-5: the truncation is h^2 / 6 times a third
    derivative of order one, 2e-11, and the rounding of the difference quotient 1e-16 / 1e-5 = 1e-11: bound 1e-8 absolute."""
    rng = np.random.default_rng(3)
    h = 1e-5
    worst = 0.0
    for _ in range(4):
        d = rng.normal(size=3)
        w = norm * d / np.linalg.norm(d)
        J = so3_right_jacobian(torch.from_numpy(w)).numpy()
        R0 = _exp(w)
        Jn = np.stack([(_log(R0.T @ _exp(w + h * e)) - _log(R0.T @ _exp(w - h * e))) / (2 * h) for e in np.eye(3)], 1)
        worst = max(worst, float(np.abs(J - Jn).max()))
    print(f"\n|omega| = {norm}: worst |Jr - central difference| = {worst:.2e} (bound 1e-8)")
    assert worst <= 1e-8
    assert so3_right_jacobian(torch.zeros(3, dtype=torch.float64)).equal(torch.eye(3, dtype=torch.float64))


def test_right_jacobian_z_column_and_the_yaw_bits():
    psi = torch.tensor([0.0, 1e-9, 0.2, -0.7, 1.0, 3.0], dtype=torch.float64)
    om = torch.zeros((6, 3), dtype=torch.float64)
    om[:, 2] = psi
    J = so3_right_jacobian(om)
    assert torch.equal(J[:, :, 2], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(6, 3))
    g = torch.from_numpy(np.random.default_rng(1).normal(size=(6, 3)))
    assert torch.equal(cm.rollout._jr_transposed(J, g)[:, 2], g[:, 2])      # the z component of plan_rot.grad is plan_yaw.grad's expression
    # rot_plan_poses on z-only vectors: yaw_plan_poses to the bit, a zero entry keeps its bits
    rng = np.random.default_rng(2)
    q = rng.normal(size=(2, 2, 4, 4))
    pose = torch.from_numpy(np.concatenate([rng.normal(size=(2, 2, 4, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32))
    yaw = torch.from_numpy(rng.uniform(-0.5, 0.5, (2, 2, 4)))
    yaw[0, 0, 0] = 0.0
    vec = torch.zeros((2, 2, 4, 3), dtype=torch.float64)
    vec[..., 2] = yaw
    got = rot_plan_poses(pose, vec)
    assert torch.equal(got.view(torch.int32), yaw_plan_poses(pose, yaw).view(torch.int32))
    assert torch.equal(got[0, 0, 0].view(torch.int32), pose[0, 0, 0].view(torch.int32))
    # a tilt: still a unit quaternion, q (x) Exp(omega) as rotation matrices
    vec[1, 1, 2] = torch.tensor([0.05, -0.1, 0.2], dtype=torch.float64)
    t = rot_plan_poses(pose, vec)[1, 1, 2, 3:].to(torch.float64).numpy()
    w, x, y, z = pose[1, 1, 2, 3:].to(torch.float64).numpy()

    def mat(w, x, y, z):
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    np.testing.assert_allclose(mat(*t), mat(w, x, y, z) @ _exp(np.array([0.05, -0.1, 0.2])), atol=1e-6)      # (float32 quaternions)


# ---- argument checks and the surface ----
def test_argument_checks_without_a_gpu():
    lib = cm._capi.lib()
    tape, g, r = cm._capi.CmpcWalkTape(), cm._capi.CmpcWalkGrads(), cm._capi.CmpcWalkGradsRot()
    assert lib.cmpc_rollout_walk_vjp_rot_device(None, M, 0, 1, C.byref(tape), 0, None, C.byref(g), C.byref(r), None) != 0
    assert lib.cmpc_rollout_walk_vjp_rot_device(None, M, 0, 1, C.byref(tape), 0, None, C.byref(g), None, None) != 0
    assert lib.cmpc_rollout_walk_vjp_rot_gate_device(None, C.byref(cm._capi.CmpcWalkGateRot()), None) != 0
    assert lib.cmpc_rollout_walk_vjp_rot_gate(None) != 0
    c, cl, cr = np.zeros((B, 9)), np.zeros((B, 2, M, 3)), np.zeros((B, 2, M, 3))
    okb, sens, status = np.zeros((B,), np.int32), np.zeros((B, wt.SENS), np.float32), np.zeros((B,), np.int32)

    def gate(base_kw=None, **kw):
        g = cm._capi.CmpcWalkGateRot()
        g.base = _base(None, **{**dict(carry_state=_ptr(c), carry_list=_ptr(cl), do_pre=1, tick_pre=0, ok_out=_ptr(okb)), **(base_kw or {})})
        g.carry_list_rot = _ptr(cr)
        for k, v in kw.items():
            setattr(g, k, v)
        return lib.cmpc_rollout_walk_vjp_rot_gate(C.byref(g))
    post = dict(do_post=1, tick_post=1, seed_state=_ptr(c), tick_state=_ptr(c), tick_list=_ptr(cl), tick_sens=_ptr(sens), status_row=_ptr(status))
    assert gate() == 0 and gate(post, tick_list_rot=_ptr(cr)) == 0
    assert gate(carry_list_rot=None) != 0                   # the third carry is required
    assert gate(post) != 0                                  # the POST part without the tick's dGradPrevListRot
    assert gate(dict(batch=0)) != 0 and gate(dict(carry_list=None)) != 0 and gate(dict(ok_out=None)) != 0 and gate(dict(do_pre=0)) != 0      # the base's own
    assert gate(dict(do_post=1)) != 0


def test_exports_struct_sizes_and_the_python_surface():
    import inspect
    lib = cm._capi.lib()
    for name in ("cmpc_rollout_walk_vjp_rot_device", "cmpc_rollout_walk_vjp_rot_gate", "cmpc_rollout_walk_vjp_rot_gate_device"):
        assert name in cm._capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(cm._capi.CmpcWalkGradsRot) == 4 * 8
    assert C.sizeof(cm._capi.CmpcWalkGateRot) == C.sizeof(cm._capi.CmpcWalkGate) + 4 * 8
    assert C.sizeof(cm._capi.CmpcWalkGrads) == 9 * 8 and C.sizeof(cm._capi.CmpcWalkGate) == 16 + 8 + 8 + 9 * 8 + 16 + 4 * 8      # the pinned layouts
    ro = cm.rollout.WalkingRollout
    assert list(inspect.signature(ro.backward_device_rot).parameters) == ["self", "w", "grad_states", "grad_X"]
    p = inspect.signature(cm.BatchSolver.rollout_walk_vjp_device).parameters
    assert all(p[k].default is None for k in ("carry_list_rot", "dGradPlanRot", "grad_rot", "removed"))
    assert hasattr(cm.BatchSolver, "rollout_walk_vjp_rot_gate_device")
    assert inspect.signature(cm.rollout_differentiable).parameters["plan_rot"].default is None
    with pytest.raises(ValueError):
        cm.rollout_differentiable(None, 1, None, plan_yaw=object(), plan_rot=object())
    with pytest.raises(NotImplementedError):      # plan_yaw stays off the device path: plan_rot[..., 2] is the way there
        cm.rollout_differentiable(None, 1, None, plan_yaw=object(), device_walk=True)
    assert "plan_rot[..., 2]" in cm.rollout_differentiable.__doc__
