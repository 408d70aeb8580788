"""ctypes bindings of include/h12learn.h (the learner-side kernels of libh12env.so) on torch tensors.

Both wrappers launch on the current HIP stream of the tensors' device, allocate only what they return and never
synchronise, so they can run inside ``torch.cuda.graph`` capture."""
from __future__ import annotations

import ctypes as C

import torch

from ._abi import H12EnvError, load_library

LEARN_SYMBOLS = ["h12learn_rms_row_chunk", "h12learn_rms_workspace_bytes", "h12learn_rms_forward",
                 "h12learn_gae_soft", "h12learn_last_error"]

_bound = None


def learn_library():
    """libh12env.so with the h12learn_* prototypes set.  A library without them is an error (no fallback)."""
    global _bound
    if _bound is not None:
        return _bound
    lib = load_library()
    vp = C.c_void_p
    for s in LEARN_SYMBOLS:
        if not hasattr(lib, s):
            raise H12EnvError(f"libh12env.so lacks {s}; rebuild it (csrc/h12_learn.hip)")
    lib.h12learn_rms_row_chunk.argtypes = []
    lib.h12learn_rms_row_chunk.restype = C.c_int
    lib.h12learn_rms_workspace_bytes.argtypes = [C.c_longlong, C.c_int]
    lib.h12learn_rms_workspace_bytes.restype = C.c_size_t
    lib.h12learn_rms_forward.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, C.c_int, C.c_float, C.c_int, vp,
                                         C.c_size_t, vp]
    lib.h12learn_rms_forward.restype = C.c_int
    lib.h12learn_gae_soft.argtypes = [vp] * 7 + [C.c_float, C.c_float, C.c_int, C.c_int, vp, vp, vp]
    lib.h12learn_gae_soft.restype = C.c_int
    lib.h12learn_last_error.argtypes = []
    lib.h12learn_last_error.restype = C.c_char_p
    _bound = lib
    return lib


def _check(lib, rc: int, what: str):
    if rc != 0:
        msg = lib.h12learn_last_error()
        raise H12EnvError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _f32(t: torch.Tensor, name: str):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: a contiguous float32 CUDA tensor is required, got {t.dtype} on {t.device}")
    return t


def rms_row_chunk() -> int:
    return learn_library().h12learn_rms_row_chunk()


def rms_workspace(n: int, d: int, device) -> torch.Tensor:
    """A zeroed workspace for rms_forward on [n][d] inputs."""
    nbytes = learn_library().h12learn_rms_workspace_bytes(n, d)
    return torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)


def rms_forward(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, count: torch.Tensor, epsilon: float,
                update: bool, workspace: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """RunningMeanStd.forward on the device: x is (n, ...) with prod(...) == mean.numel(); mean, var, count are
    updated in place when ``update``; returns the normalised tensor (``out`` may be x itself)."""
    lib = learn_library()
    _f32(x, "x"), _f32(mean, "mean"), _f32(var, "var"), _f32(count, "count")
    n, d = x.shape[0], mean.numel()
    if n < 1 or x.numel() != n * d or var.numel() != d or count.numel() != 1:
        raise ValueError(f"rms_forward: x {tuple(x.shape)} does not match statistics of {d} columns")
    y = torch.empty_like(x) if out is None else _f32(out, "out")
    if y.shape != x.shape:
        raise ValueError("rms_forward: out must have x's shape")
    ws_ptr, ws_bytes = None, 0
    if update:
        if workspace is None:
            raise ValueError("rms_forward: update needs a workspace (rms_workspace)")
        ws_ptr, ws_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    _check(lib, lib.h12learn_rms_forward(x.data_ptr(), y.data_ptr(), mean.data_ptr(), var.data_ptr(),
                                         count.data_ptr(), n, d, float(epsilon), int(bool(update)), ws_ptr, ws_bytes,
                                         _stream(x.device)), "h12learn_rms_forward")
    return y


def gae_soft(rewards, values, dones, true_dones, next_value, next_done, next_true_done, gamma: float,
             gae_lambda: float):
    """(advantages, returns) of the CaT GAE; [T][N] inputs, [N] bootstrap inputs."""
    lib = learn_library()
    T, N = rewards.shape
    for name, t in (("rewards", rewards), ("values", values), ("dones", dones), ("true_dones", true_dones)):
        if _f32(t, name).shape != (T, N):
            raise ValueError(f"gae_soft: {name} must be ({T}, {N})")
    for name, t in (("next_value", next_value), ("next_done", next_done), ("next_true_done", next_true_done)):
        if _f32(t, name).numel() != N:
            raise ValueError(f"gae_soft: {name} must have {N} elements")
    adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    # gamma * lambda is formed in double and narrowed once, as torch narrows the product of the Python scalars
    _check(lib, lib.h12learn_gae_soft(rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), true_dones.data_ptr(),
                                      next_value.data_ptr(), next_done.data_ptr(), next_true_done.data_ptr(),
                                      float(gamma), float(gamma) * float(gae_lambda), T, N, adv.data_ptr(),
                                      ret.data_ptr(), _stream(rewards.device)), "h12learn_gae_soft")
    return adv, ret
