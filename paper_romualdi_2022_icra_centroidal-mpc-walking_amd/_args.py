"""The one check between a torch tensor and the raw pointer a kernel is given.  ptr and out raise AssertionError themselves, so the refusals hold
under `python -O` as well; the text is "{name}: expected {dtype} {shape}" unless the caller has one of its own (msg).  An entry of `shape` that is None
stands for any length of that axis.  Also here, because every solver module needs them and this module imports none of them: opt_ptr and _upload."""
import numpy as np

_torch = None   # (the torch module, imported by the first call that allocates)


def _wild(got, shape):
    """the shape test for a `shape` that is not the tensor's own tuple: one with None entries (or a list)"""
    return len(got) == len(shape) and all(w is None or w == g for w, g in zip(shape, got))


def _fits(t, dtype, shape):
    """t is a contiguous CUDA tensor of `dtype` and `shape`"""
    return t.is_cuda and t.dtype == dtype and t.is_contiguous() and (tuple(t.shape) == shape or _wild(t.shape, shape))


def ptr(t, dtype, shape, name, required=False, msg=None):
    """data_ptr of an optional CUDA tensor (None -> NULL; required: None is refused too), checked (_fits written out: this is on every call's path)"""
    if t is None:
        if not required:
            return None
    elif t.is_cuda and t.dtype == dtype and t.is_contiguous() and (tuple(t.shape) == shape or _wild(t.shape, shape)):
        return t.data_ptr()
    raise AssertionError(msg or f"{name}: expected {dtype} {tuple(shape)}")


def out(t, dtype, shape, name, device, msg=None):
    """the output tensor: torch.empty when t is None, else t, checked"""
    if t is None:
        global _torch
        if _torch is None:
            import torch as _torch
        return _torch.empty(shape, dtype=dtype, device=device)
    if _fits(t, dtype, shape):
        return t
    raise AssertionError(msg or f"{name}: expected {dtype} {tuple(shape)}")


def opt_ptr(t):
    """data_ptr of an optional tensor (None -> NULL), unchecked"""
    return t.data_ptr() if t is not None else None


def _upload(a, dev, dtype, hold):
    """`a` on the device in `dtype` for launches that are queued and not waited for: a torch tensor is cast as it is; anything else goes through a host
    tensor appended to `hold` and a copy the host does not wait for, so `hold` has to outlive that copy (WalkingRollout._walk_inputs, a builder
    dict's "_host")"""
    import torch
    if isinstance(a, torch.Tensor):
        return a.detach().to(dev, dtype)
    hold.append(torch.from_numpy(np.ascontiguousarray(a, str(dtype).split(".")[1])))
    return hold[-1].to(dev, non_blocking=True)
