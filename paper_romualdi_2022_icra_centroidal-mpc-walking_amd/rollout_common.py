"""What the modules of the roll-out layer share, in a module that imports none of them (which module holds what: DESIGN.md 1): the check that stands
where an `assert` stood, the conversion of "numpy array or tensor", the argument binding behind pinned signatures, the refusals that more than one
method raises, the launch-stream helper and the zero allocator -- ONE of each (tests/test_rollout_args_cpu.py); walk_schedule and plan_speed."""
import inspect

import numpy as np

from ._args import ptr


def need(cond, text):
    """what `assert cond, text` says, raised under `python -O` too"""
    if not cond:
        raise AssertionError(text)


def walk_schedule(ticks, every, replan=(), tick0=0):
    """The calls of a checkpointed walk of ticks tick0 .. tick0 + ticks - 1 -- a pure function.  The walk is cut at the multiples of `every` (tick numbers,
    not counted from tick0) and at the replan ticks that lie strictly inside it.  -> (calls, snapshots): calls = [(t0, t1), ...], half-open and in order;
    snapshots = the ticks k * every, k >= 1, strictly inside the walk: each is the first tick of a call, and the snapshot is taken in front of it.
    every None, or at or beyond the walk's end: no snapshot."""
    tick0, end = int(tick0), int(tick0) + int(ticks)
    need(ticks >= 1 and tick0 >= 0 and (every is None or int(every) >= 1), "walk_schedule: ticks >= 1, tick0 >= 0, every >= 1")
    snaps = [] if every is None else [t for t in range(int(every), end, int(every)) if t > tick0]
    cuts = sorted({tick0, end} | set(snaps) | {int(t) for t in replan if tick0 < int(t) < end})
    return list(zip(cuts[:-1], cuts[1:])), snaps


def plan_speed(plan):
    """the mean walking speed of a plan: the CoM reference's when no com_speed is given"""
    last = max(c.position[0] for lst in plan.values() for c in lst)
    t_last = max(c.activation_time for lst in plan.values() for c in lst)
    return last / t_last if t_last > 0 else 0.0


def tensor(a, dev, dtype, host_dtype=None):
    """numpy array or tensor -> contiguous tensor of `dtype` on `dev`, no copy where it is one; host_dtype: the host array is cast on the host first"""
    import torch
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.asarray(a) if host_dtype is None else np.ascontiguousarray(a, host_dtype))
    return a.to(dev, dtype).contiguous()


def seed(a, dev, dtype, shape, name, msg=None):
    """tensor(a, dev, dtype) through _args.ptr's check of dtype and shape (its text, or msg(tensor) where the caller has a text of its own)"""
    t = tensor(a, dev, dtype)
    ptr(t, dtype, shape, name, True, msg(t) if msg and tuple(t.shape) != tuple(shape) else None)
    return t


def direction(a, dev, B, dtype, tail, lead=()):
    """one group of forward-mode directions (None: zero, stays None) as a tensor [*lead, B, k, *tail], the k columns right behind B"""
    if a is None:
        return None
    a = tensor(a, dev, dtype)
    if not (a.dim() == len(lead) + 2 + len(tail) and tuple(a.shape[:len(lead) + 1]) == lead + (B,) and tuple(a.shape[len(lead) + 2:]) == tail):
        raise AssertionError(f"direction of shape {tuple(a.shape)}: expected {lead + (B, 'k') + tail}")
    return a


def bound(method, *args, **kwargs):
    """the arguments of a call of `method`, defaults filled in: .args and .kwargs are what the method's driver is given"""
    call = inspect.signature(method).bind(*args, **kwargs)
    call.apply_defaults()
    return call


def refuse_long_lists(who, M, why=" of a refill walk"):
    if M > 16:
        raise NotImplementedError(f"{who}: lists longer than 16 contacts are out of scope{why}")


def refuse_push_and_wrench_trials(who, push, wrench_trials):
    if push is not None and wrench_trials is not None:
        raise ValueError(f"{who}: push or wrench_trials, not both")


def refuse_push_with_sensor(sensor, push):
    if sensor is not None and push is not None:
        raise ValueError("push= with a sensor: a known push and a sensed one are not summed (hidden_wrench is what the sensor reads)")


class LaunchStream:
    def _on_launch_stream(self, fn):
        """fn() with the solver's launch stream as torch's current stream; the caller's stream waits behind it whether fn returns or raises"""
        torch = self.torch
        ls = self.solver.launch_stream
        cur = torch.cuda.current_stream(self.dev)
        ls.wait_stream(cur)
        try:
            with torch.cuda.stream(ls):
                return fn()
        finally:
            cur.wait_stream(ls)

    def _queued(self, fn):
        """fn() with the solver's launch stream as torch's current stream, as walk_device queues its ticks"""
        need(self.retry != "launch", "the device walk needs retry='kernel' or None")
        return self._on_launch_stream(fn)

    def _z(self, shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float64, device=self.dev)
