"""The argument checks of BatchSolver on the device (_args.py): one handle, B = 2, N = 10, lists of 2 contacts, k = 2, a taped walk of 3 ticks.  One
method per module and per family is called with an otherwise valid argument set in which one CUDA tensor is, in turn, of the other precision, one element
short in its last axis, a non-contiguous view of the right shape, and a host tensor.  Each such call must end in Python -- AssertionError naming the
argument -- with the library not touched: while it runs the handle's library is a proxy that records and refuses every attribute read.  Nothing here
launches with a malformed argument.  Then the valid call runs on the real library and, where the method has a twin, agrees with it bit for bit."""
import numpy as np
import pytest

import cmpc_amd as cm
from tests.test_gpu_walk_record import _start

pytestmark = pytest.mark.gpu

B, N, K, T = 2, 10, 2, 3


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b, msg=""):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


class _Untouchable:
    """in the place of the library: every attribute read is recorded and refused"""

    def __init__(self):
        self.touched = []

    def __getattr__(self, name):
        self.touched.append(name)
        raise RuntimeError(f"the library was touched: {name}")


@pytest.fixture(scope="module")
def st():
    import torch
    cfg = cm.config.ergocub_gazebo_v1(N, 0.06)
    ro = cm.rollout.WalkingRollout(cfg, B, plan=cm.rollout.walking_plan(cfg, steps=0))
    assert ro.M == 2
    com0, dcom0, h0, _ = _start(B)
    w = ro.walk_device_taped(T, com0, dcom0, h0)
    torch.cuda.synchronize()
    assert (w["end_tick"].cpu().numpy() == -1).all()
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda shape, dt=torch.float64: torch.randn(shape, generator=g, dtype=torch.float64).to(dt).to(ro.dev)
    yield dict(ro=ro, s=ro.solver, L=ro.L, M=ro.M, dev=ro.dev, tape=w["tape"], end_tick=w["end_tick"], rnd=rnd)
    ro.solver.close()


def _walk_vjp_args(st):
    import torch
    s, L, M, rnd = st["s"], st["L"], st["M"], st["rnd"]
    gS = rnd((T + 1, B, 9))
    return dict(grad_states=gS, carry_state=gS[T].clone(), carry_list=torch.zeros((B, 2, M, 3), dtype=torch.float64, device=st["dev"]),
                status=torch.zeros((T, B), dtype=torch.int32, device=st["dev"]), grad_X=rnd((T, B, L.nx), torch.float32),
                wrench=torch.zeros((T, B, N, 6), dtype=torch.float32, device=st["dev"]))


def _cases(st):
    """name -> (call(**tensors), the valid tensors, the one that is spoilt)"""
    import torch
    s, L, M, tp, rnd, dev = st["s"], st["L"], st["M"], st["tape"], st["rnd"], st["dev"]
    f32 = torch.float32
    X, P, lam, state = tp["X"][0], tp["P"][0], tp["lam_g"][0], tp["states"][0]
    now1 = 0.06
    lists1 = dict(list_t=tp["list_t"][1], list_n=tp["list_n"][1], land=tp["land"][1], plan=(tp["plan_t"][1], tp["plan_n"][1]),
                  prev=(tp["list_t"][0], tp["list_n"][0]), ok=tp["ok"][1])
    va = _walk_vjp_args(st)
    head = (0, T, tp, 0, st["end_tick"])
    walk_vjp = lambda grad_states, carry_state, carry_list, status, grad_X, wrench: s.rollout_walk_vjp_device(
        *head, grad_states, carry_state, carry_list, status, grad_X=grad_X, wrench=wrench)
    walk_vjp_rows = lambda grad_states, carry_state, carry_list, status, grad_X, wrench: s.rollout_walk_vjp_rows_device(
        *head, grad_states, carry_state, carry_list, status, grad_X=grad_X, wrench=wrench)
    z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    return {
        "solve_device": (lambda dP, dX0: s.solve_device(dP, dX0), dict(dP=P, dX0=s.cold_start_device(P)), "dP"),
        "multipliers_device": (lambda dX, dP: s.multipliers_device(dX, dP), dict(dX=X, dP=P), "dX"),
        "solution_jvp_rot_device": (lambda dDirP, dDirRot: s.solution_jvp_rot_device(X, P, lam, dDirP=dDirP, dDirRot=dDirRot),
                                    dict(dDirP=rnd((B, K, L.np), f32), dDirRot=rnd((B, K, 2, N, 3))), "dDirRot"),
        "solution_vjp_cols_device": (lambda dGradX: s.solution_vjp_cols_device(X, P, lam, dGradX), dict(dGradX=rnd((B, K, L.nx), f32)), "dGradX"),
        "plant_step_jvp_device": (lambda dDirState, dDirX: s.plant_step_jvp_device(X, P, state, dDirState, dDirX=dDirX),
                                  dict(dDirState=rnd((B, 9)), dDirX=rnd((B, L.nx), f32)), "dDirState"),
        "contacts_position_vjp_device": (lambda list_t, dGradListOut: s.contacts_position_vjp_device(now1, dGradListOut=dGradListOut, phase=2,
                                                                                                     **dict(lists1, list_t=list_t)),
                                         dict(list_t=lists1["list_t"], dGradListOut=rnd((B, 2, M, 3))), "list_t"),
        "cold_start_device": (lambda dP: s.cold_start_device(dP), dict(dP=P), "dP"),
        "rollout_walk_vjp_device": (walk_vjp, va, "grad_states"),
        "rollout_walk_vjp_rows_device": (walk_vjp_rows, va, "grad_states"),
        "rollout_walk_jvp_device": (lambda dir_states, carry_list, status: s.rollout_walk_jvp_device(*head, K, dir_states, carry_list, status),
                                    dict(dir_states=rnd((T + 1, B, K, 9)), carry_list=z((B, K, 2, M, 3)), status=z((T, B), torch.int32)), "dir_states"),
        "walk_snapshot": (lambda state: s.walk_snapshot(T, 0, M, tensors=dict(state=state)), dict(state=state), "state"),
        "walk_measures_vjp_device": (lambda grad_measures, grad_states, grad_X, direct: s.walk_measures_vjp_device(*head, grad_measures, grad_states,
                                                                                                                   grad_X, direct),
                                     dict(grad_measures=rnd((T, B, 4)), grad_states=z((T + 1, B, 9)), grad_X=z((T, B, L.nx), f32), direct=z((T, B, 32))),
                                     "grad_measures"),
    }


NAMES = ("solve_device", "multipliers_device", "solution_jvp_rot_device", "solution_vjp_cols_device", "plant_step_jvp_device",
         "contacts_position_vjp_device", "cold_start_device", "rollout_walk_vjp_device", "rollout_walk_vjp_rows_device", "rollout_walk_jvp_device",
         "walk_snapshot", "walk_measures_vjp_device")


def _spoilt(t):
    """the four malformed stand-ins of a CUDA tensor"""
    import torch
    other = {torch.float32: torch.float64, torch.float64: torch.float32, torch.int32: torch.int64}[t.dtype]
    view = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)[..., ::2]
    assert tuple(view.shape) == tuple(t.shape) and not view.is_contiguous()
    return {"the other precision": t.to(other), "one short in the last axis": t[..., :-1].contiguous(), "a non-contiguous view": view, "a host tensor": t.cpu()}


@pytest.mark.parametrize("name", NAMES)
def test_malformed_tensor_is_refused_in_python_and_the_valid_call_runs(st, name):
    import torch
    s = st["s"]
    call, good, which = _cases(st)[name]
    torch.cuda.synchronize()
    lib, proxy = s._lib, _Untouchable()
    for what, bad in _spoilt(good[which]).items():
        s._lib = proxy
        try:
            with pytest.raises(AssertionError, match=which):
                call(**dict(good, **{which: bad}))
        finally:
            s._lib = lib
        assert proxy.touched == [], f"{name}, {what}: {proxy.touched}"
    with torch.cuda.stream(s.launch_stream):
        call(**{k: v.clone() for k, v in good.items()})
    torch.cuda.synchronize()


def test_valid_calls_agree_with_their_twins_bit_for_bit(st):
    import torch
    s, L, M, tp, rnd = st["s"], st["L"], st["M"], st["tape"], st["rnd"]
    X, P, lam = tp["X"][0], tp["P"][0], tp["lam_g"][0]
    # the reverse walk through rows with tick0 == row0 on a whole-walk tape is the whole-walk call
    va = _walk_vjp_args(st)
    outs = []
    with torch.cuda.stream(s.launch_stream):
        for method in (s.rollout_walk_vjp_device, s.rollout_walk_vjp_rows_device):
            a = {k: v.clone() for k, v in va.items()}
            method(0, T, tp, 0, st["end_tick"], a["grad_states"], a["carry_state"], a["carry_list"], a["status"], grad_X=a["grad_X"], wrench=a["wrench"])
            outs.append(a)
        # the solution JVPs without the later families' directions, each through its own C symbol
        dp = rnd((B, K, L.np), torch.float32)
        j0, s0 = s.solution_jvp_device(X, P, lam, dp)
        j1, s1 = s.solution_jvp_model_device(X, P, lam, dDirP=dp)
        j2, s2 = s.solution_jvp_rot_device(X, P, lam, dDirP=dp)
        # the cotangent columns against the single-cotangent calls
        gx = rnd((B, K, L.nx), torch.float32)
        cp, _, _, cs = s.solution_vjp_cols_device(X, P, lam, gx)
        singles = [s.solution_vjp_rot_device(X, P, lam, gx[:, j].contiguous(), grad_model=False) for j in range(K)]
        plain = [s.solution_vjp_device(X, P, lam, gx[:, j].contiguous()) for j in range(K)]
        # the two list-path adjoints on the same tape arguments
        lists1 = dict(list_t=tp["list_t"][1], list_n=tp["list_n"][1], land=tp["land"][1], plan=(tp["plan_t"][1], tp["plan_n"][1]),
                      prev=(tp["list_t"][0], tp["list_n"][0]), ok=tp["ok"][1])
        _, st_pos = s.contacts_position_vjp_device(0.06, dGradListOut=rnd((B, 2, M, 3)), phase=2, **lists1)      # (phase 2: the sample + merge part)
        _, st_rot = s.contacts_orientation_vjp_device(0.06, dGradListRotOut=rnd((B, 2, M, 3)), **lists1)
    torch.cuda.synchronize()
    for k in va:
        _same_bits(outs[0][k], outs[1][k], f"rows against whole walk: {k}")
    assert (outs[0]["status"].cpu().numpy() == 0).all() and float(outs[0]["carry_state"].abs().max()) > 0
    assert not np.array_equal(_bits(outs[0]["carry_state"]), _bits(va["carry_state"]))
    assert (s0.cpu().numpy()[:, 0] == 0).all() and float(j0.abs().max()) > 0
    _same_bits(j1, j0, "solution_jvp_model_device without model directions")
    _same_bits(j2, j1, "solution_jvp_rot_device without rotation directions")
    assert (cs.cpu().numpy()[:, 0] == 0).all() and float(cp.abs().max()) > 0
    for j in range(K):
        _same_bits(cp[:, j], singles[j][2], f"column {j} against solution_vjp_rot_device")
        _same_bits(singles[j][2], plain[j][0], f"column {j}: solution_vjp_rot_device against solution_vjp_device")
    # (no bit-for-bit relation between these two: they share their tape arguments, and on the same valid tape both must report every problem clean)
    assert st_pos.cpu().numpy().tolist() == st_rot.cpu().numpy().tolist() == [0] * B
