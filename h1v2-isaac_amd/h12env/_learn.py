"""ctypes bindings of include/h12learn.h (the learner-side kernels of libh12env.so) on torch tensors.

The wrappers launch on the current HIP stream of the tensors' device, allocate only what they return and never
synchronise, so they can run inside ``torch.cuda.graph`` capture."""
from __future__ import annotations

import ctypes as C

import torch

from ._abi import H12EnvError, load_library

LEARN_SYMBOLS = ["h12learn_rms_row_chunk", "h12learn_rms_workspace_bytes", "h12learn_rms_forward",
                 "h12learn_gae_soft", "h12learn_mlp_max_width", "h12learn_mlp_packed_bytes", "h12learn_mlp_pack",
                 "h12learn_mlp_forward", "h12learn_mirror_rows", "h12learn_mlp_train_rows",
                 "h12learn_mlp_train_max_width", "h12learn_mlp_packed_t_bytes", "h12learn_mlp_pack_t",
                 "h12learn_mlp_forward_train", "h12learn_mlp_backward_workspace_bytes", "h12learn_mlp_backward",
                 "h12learn_ppo_head_rows", "h12learn_ppo_head_max_actions", "h12learn_ppo_head_workspace_bytes",
                 "h12learn_ppo_head", "h12learn_cleanrl_head_rows", "h12learn_cleanrl_head_workspace_bytes",
                 "h12learn_cleanrl_head", "h12learn_lstm_max_hidden", "h12learn_lstm_packed_bytes",
                 "h12learn_lstm_pack", "h12learn_lstm_step", "h12learn_lstm_seq_packed_bytes",
                 "h12learn_lstm_seq_pack", "h12learn_lstm_seq_forward", "h12learn_lstm_seq_backward",
                 "h12learn_rnd_reward", "h12learn_rnd_finish", "h12learn_optim_chunk", "h12learn_optim_max_tensors",
                 "h12learn_optim_fold", "h12learn_optim_workspace_bytes", "h12learn_optim_step", "h12learn_last_error"]

MLP_MAX_NETS = 4
MLP_MAX_LAYERS = 8
MLP_NORM_NONE, MLP_NORM_VAR, MLP_NORM_STD = 0, 1, 2


class MlpNet(C.Structure):
    """h12learn_mlp_net"""
    _fields_ = [("n_layers", C.c_int), ("dims", C.c_int * (MLP_MAX_LAYERS + 1)), ("W", C.c_void_p * MLP_MAX_LAYERS),
                ("b", C.c_void_p * MLP_MAX_LAYERS)]


class MlpDesc(C.Structure):
    """h12learn_mlp_desc"""
    _fields_ = [("n_nets", C.c_int), ("d_in", C.c_int), ("norm_kind", C.c_int), ("norm_eps", C.c_float),
                ("norm_mean", C.c_void_p), ("norm_scale", C.c_void_p), ("nets", MlpNet * MLP_MAX_NETS)]


LSTM_MAX_NETS = 2


class LstmCell(C.Structure):
    """h12learn_lstm_cell"""
    _fields_ = [("w_ih", C.c_void_p), ("w_hh", C.c_void_p), ("b_ih", C.c_void_p), ("b_hh", C.c_void_p)]


class LstmDesc(C.Structure):
    """h12learn_lstm_desc"""
    _fields_ = [("d_in", C.c_int), ("hidden", C.c_int), ("norm_kind", C.c_int), ("norm_eps", C.c_float),
                ("norm_mean", C.c_void_p), ("norm_scale", C.c_void_p), ("cells", LstmCell * LSTM_MAX_NETS),
                ("mlp", MlpDesc)]


class LstmIo(C.Structure):
    """h12learn_lstm_io"""
    _fields_ = [("x", C.c_void_p), ("reset", C.c_void_p), ("n", C.c_longlong), ("h_in", C.c_void_p * LSTM_MAX_NETS),
                ("c_in", C.c_void_p * LSTM_MAX_NETS), ("h_out", C.c_void_p * LSTM_MAX_NETS),
                ("c_out", C.c_void_p * LSTM_MAX_NETS), ("y", C.c_void_p * LSTM_MAX_NETS)]


class LstmSeqDesc(C.Structure):
    """h12learn_lstm_seq_desc"""
    _fields_ = [("n_nets", C.c_int), ("hidden", C.c_int), ("w_hh", C.c_void_p * LSTM_MAX_NETS)]


class LstmSeqIo(C.Structure):
    """h12learn_lstm_seq_io"""
    _fields_ = [("T", C.c_int), ("reserved", C.c_int), ("n", C.c_longlong), ("dones", C.c_void_p),
                ("zx", C.c_void_p * LSTM_MAX_NETS), ("h0", C.c_void_p * LSTM_MAX_NETS),
                ("c0", C.c_void_p * LSTM_MAX_NETS), ("h_seq", C.c_void_p * LSTM_MAX_NETS),
                ("c_seq", C.c_void_p * LSTM_MAX_NETS), ("gates", C.c_void_p * LSTM_MAX_NETS)]


class LstmSeqGradIo(C.Structure):
    """h12learn_lstm_seq_grad_io"""
    _fields_ = [("T", C.c_int), ("reserved", C.c_int), ("n", C.c_longlong), ("dones", C.c_void_p),
                ("dh_seq", C.c_void_p * LSTM_MAX_NETS), ("gates", C.c_void_p * LSTM_MAX_NETS),
                ("c_seq", C.c_void_p * LSTM_MAX_NETS), ("c0", C.c_void_p * LSTM_MAX_NETS),
                ("dz", C.c_void_p * LSTM_MAX_NETS), ("dh0", C.c_void_p * LSTM_MAX_NETS),
                ("dc0", C.c_void_p * LSTM_MAX_NETS)]


PPO_STD_SCALAR, PPO_STD_LOG = 0, 1


class PpoHeadArgs(C.Structure):
    """h12learn_ppo_head_args"""
    _fields_ = [("m", C.c_longlong), ("B", C.c_longlong), ("n_src", C.c_longlong), ("A", C.c_int), ("std_kind", C.c_int),
                ("actions_direct", C.c_int), ("use_clipped_value_loss", C.c_int), ("mean", C.c_void_p),
                ("value", C.c_void_p), ("std_param", C.c_void_p), ("idx", C.c_void_p), ("old_log_prob", C.c_void_p),
                ("advantages", C.c_void_p), ("returns", C.c_void_p), ("target_values", C.c_void_p),
                ("old_mu", C.c_void_p), ("old_sigma", C.c_void_p), ("actions", C.c_void_p), ("clip_param", C.c_double),
                ("value_loss_coef", C.c_double), ("entropy_coef", C.c_double), ("desired_kl", C.c_double),
                ("d_mean", C.c_void_p), ("d_value", C.c_void_p), ("d_param", C.c_void_p), ("out", C.c_void_p),
                ("lr", C.c_void_p), ("stats_accum", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


class CleanRlHeadArgs(C.Structure):
    """h12learn_cleanrl_head_args"""
    _fields_ = [("m", C.c_longlong), ("n_src", C.c_longlong), ("A", C.c_int), ("norm_adv", C.c_int),
                ("clip_vloss", C.c_int), ("reserved", C.c_int), ("mean", C.c_void_p), ("value", C.c_void_p),
                ("logstd", C.c_void_p), ("idx", C.c_void_p), ("old_log_prob", C.c_void_p), ("advantages", C.c_void_p),
                ("returns_n", C.c_void_p), ("values_n", C.c_void_p), ("actions", C.c_void_p),
                ("value_mean", C.c_void_p), ("value_var", C.c_void_p), ("value_eps", C.c_double),
                ("clip_coef", C.c_double), ("ent_coef", C.c_double), ("vf_coef", C.c_double), ("d_mean", C.c_void_p),
                ("d_value", C.c_void_p), ("d_logstd", C.c_void_p), ("out", C.c_void_p), ("stats_accum", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class RndFinishArgs(C.Structure):
    """h12learn_rnd_finish_args"""
    _fields_ = [("n", C.c_longlong), ("normalize", C.c_int), ("gamma", C.c_float), ("until", C.c_longlong),
                ("err", C.c_void_p), ("ext_reward", C.c_void_p), ("weight", C.c_void_p), ("avg", C.c_void_p),
                ("mean", C.c_void_p), ("var", C.c_void_p), ("std", C.c_void_p), ("count", C.c_void_p),
                ("first", C.c_void_p), ("intrinsic", C.c_void_p), ("total", C.c_void_p)]


OPTIM_ADAM, OPTIM_RADAM = 0, 1


class OptimArgs(C.Structure):
    """h12learn_optim_args"""
    _fields_ = [("rule", C.c_int), ("n_tensors", C.c_int), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("max_norm", C.c_double), ("lr", C.c_double), ("lr_dev", C.c_void_p),
                ("p", C.POINTER(C.c_void_p)), ("g", C.POINTER(C.c_void_p)), ("exp_avg", C.POINTER(C.c_void_p)),
                ("exp_avg_sq", C.POINTER(C.c_void_p)), ("step", C.POINTER(C.c_void_p)),
                ("numel", C.POINTER(C.c_longlong)), ("grad_norm", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


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
    lib.h12learn_mlp_max_width.argtypes = []
    lib.h12learn_mlp_max_width.restype = C.c_int
    lib.h12learn_mlp_packed_bytes.argtypes = [C.POINTER(MlpDesc)]
    lib.h12learn_mlp_packed_bytes.restype = C.c_size_t
    lib.h12learn_mlp_pack.argtypes = [C.POINTER(MlpDesc), vp, vp]
    lib.h12learn_mlp_pack.restype = C.c_int
    lib.h12learn_mlp_forward.argtypes = [C.POINTER(MlpDesc), vp, vp, C.c_longlong, C.POINTER(C.c_void_p), vp]
    lib.h12learn_mlp_forward.restype = C.c_int
    lib.h12learn_mirror_rows.argtypes = [vp, C.c_longlong, vp, C.c_longlong, C.c_int, vp, C.c_int, vp, vp]
    lib.h12learn_mirror_rows.restype = C.c_int
    lib.h12learn_mlp_train_rows.argtypes = []
    lib.h12learn_mlp_train_rows.restype = C.c_int
    lib.h12learn_mlp_train_max_width.argtypes = []
    lib.h12learn_mlp_train_max_width.restype = C.c_int
    lib.h12learn_mlp_packed_t_bytes.argtypes = [C.POINTER(MlpDesc)]
    lib.h12learn_mlp_packed_t_bytes.restype = C.c_size_t
    lib.h12learn_mlp_pack_t.argtypes = [C.POINTER(MlpDesc), vp, vp]
    lib.h12learn_mlp_pack_t.restype = C.c_int
    lib.h12learn_mlp_forward_train.argtypes = [C.POINTER(MlpDesc), vp, vp, C.c_longlong, vp, C.POINTER(C.c_void_p), vp]
    lib.h12learn_mlp_forward_train.restype = C.c_int
    lib.h12learn_mlp_backward_workspace_bytes.argtypes = [C.POINTER(MlpDesc), C.c_longlong]
    lib.h12learn_mlp_backward_workspace_bytes.restype = C.c_size_t
    lib.h12learn_mlp_backward.argtypes = [C.POINTER(MlpDesc), vp, vp, C.POINTER(C.c_void_p), C.c_longlong,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), vp, vp, C.c_size_t, vp]
    lib.h12learn_mlp_backward.restype = C.c_int
    lib.h12learn_ppo_head_rows.argtypes = []
    lib.h12learn_ppo_head_rows.restype = C.c_int
    lib.h12learn_ppo_head_max_actions.argtypes = []
    lib.h12learn_ppo_head_max_actions.restype = C.c_int
    lib.h12learn_ppo_head_workspace_bytes.argtypes = [C.c_longlong, C.c_int]
    lib.h12learn_ppo_head_workspace_bytes.restype = C.c_size_t
    lib.h12learn_ppo_head.argtypes = [C.POINTER(PpoHeadArgs), vp]
    lib.h12learn_ppo_head.restype = C.c_int
    lib.h12learn_cleanrl_head_rows.argtypes = []
    lib.h12learn_cleanrl_head_rows.restype = C.c_int
    lib.h12learn_cleanrl_head_workspace_bytes.argtypes = [C.c_longlong, C.c_int]
    lib.h12learn_cleanrl_head_workspace_bytes.restype = C.c_size_t
    lib.h12learn_cleanrl_head.argtypes = [C.POINTER(CleanRlHeadArgs), vp]
    lib.h12learn_cleanrl_head.restype = C.c_int
    lib.h12learn_lstm_max_hidden.argtypes = []
    lib.h12learn_lstm_max_hidden.restype = C.c_int
    lib.h12learn_lstm_packed_bytes.argtypes = [C.POINTER(LstmDesc)]
    lib.h12learn_lstm_packed_bytes.restype = C.c_size_t
    lib.h12learn_lstm_pack.argtypes = [C.POINTER(LstmDesc), vp, vp]
    lib.h12learn_lstm_pack.restype = C.c_int
    lib.h12learn_lstm_step.argtypes = [C.POINTER(LstmDesc), vp, C.POINTER(LstmIo), vp]
    lib.h12learn_lstm_step.restype = C.c_int
    lib.h12learn_lstm_seq_packed_bytes.argtypes = [C.POINTER(LstmSeqDesc)]
    lib.h12learn_lstm_seq_packed_bytes.restype = C.c_size_t
    lib.h12learn_lstm_seq_pack.argtypes = [C.POINTER(LstmSeqDesc), vp, vp]
    lib.h12learn_lstm_seq_pack.restype = C.c_int
    lib.h12learn_lstm_seq_forward.argtypes = [C.POINTER(LstmSeqDesc), vp, C.POINTER(LstmSeqIo), vp]
    lib.h12learn_lstm_seq_forward.restype = C.c_int
    lib.h12learn_lstm_seq_backward.argtypes = [C.POINTER(LstmSeqDesc), vp, C.POINTER(LstmSeqGradIo), vp]
    lib.h12learn_lstm_seq_backward.restype = C.c_int
    lib.h12learn_rnd_reward.argtypes = [C.POINTER(MlpDesc), vp, vp, C.c_longlong, vp, vp, C.POINTER(C.c_void_p), vp]
    lib.h12learn_rnd_reward.restype = C.c_int
    lib.h12learn_rnd_finish.argtypes = [C.POINTER(RndFinishArgs), vp]
    lib.h12learn_rnd_finish.restype = C.c_int
    for q in ("h12learn_optim_chunk", "h12learn_optim_max_tensors", "h12learn_optim_fold"):
        getattr(lib, q).argtypes = []
        getattr(lib, q).restype = C.c_int
    lib.h12learn_optim_workspace_bytes.argtypes = [C.POINTER(C.c_longlong), C.c_int]
    lib.h12learn_optim_workspace_bytes.restype = C.c_size_t
    lib.h12learn_optim_step.argtypes = [C.POINTER(OptimArgs), vp]
    lib.h12learn_optim_step.restype = C.c_int
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


def mirror_rows(x: torch.Tensor, table: torch.Tensor, idx: torch.Tensor | None = None, both: bool = False,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """One launch: the rows ``idx`` (every row when None) of x [n_src][d] under the column map ``table`` (int32 [d],
    src | flip << 31; h12env.symmetry.MirrorTable.packed).  ``both``: the 2n-row concatenation (gathered, mirrored)."""
    lib = learn_library()
    _f32(x, "x")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"mirror_rows: x {tuple(x.shape)} is not (n_src >= 1, d >= 1)")
    n_src, d = x.shape
    if not (table.is_cuda and table.dtype == torch.int32 and table.is_contiguous() and table.shape == (d,)):
        raise ValueError(f"mirror_rows: table must be a contiguous int32 CUDA tensor of {d} entries")
    n = n_src
    if idx is not None:
        if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 1):
            raise ValueError("mirror_rows: idx must be a contiguous 1-D int64 CUDA tensor")
        n = idx.shape[0]
    rows = 2 * n if both else n
    if out is None:
        out = torch.empty((rows, d), dtype=torch.float32, device=x.device)
    elif _f32(out, "out").shape != (rows, d):
        raise ValueError(f"mirror_rows: out must be ({rows}, {d})")
    if n == 0:
        return out
    _check(lib, lib.h12learn_mirror_rows(x.data_ptr(), n_src, None if idx is None else idx.data_ptr(), n, d,
                                         table.data_ptr(), int(bool(both)), out.data_ptr(), _stream(x.device)),
           "h12learn_mirror_rows")
    return out


def mlp_max_width() -> int:
    return learn_library().h12learn_mlp_max_width()


def mlp_desc(nets, norm_kind: int = MLP_NORM_NONE, norm_mean: torch.Tensor | None = None,
             norm_scale: torch.Tensor | None = None, norm_eps: float = 0.0) -> MlpDesc:
    """The descriptor of ``nets``: a list of networks, each a list of (weight [out][in], bias [out]) tensor pairs.
    Shapes and data pointers only; the caller keeps the tensors alive and in place."""
    if not 1 <= len(nets) <= MLP_MAX_NETS:
        raise ValueError(f"mlp_desc: {len(nets)} networks (1..{MLP_MAX_NETS})")
    d = MlpDesc()
    d.n_nets = len(nets)
    d.d_in = int(nets[0][0][0].shape[1])
    d.norm_kind, d.norm_eps = int(norm_kind), float(norm_eps)
    if norm_kind != MLP_NORM_NONE:
        d.norm_mean, d.norm_scale = norm_mean.data_ptr(), norm_scale.data_ptr()
    for i, layers in enumerate(nets):
        if not 1 <= len(layers) <= MLP_MAX_LAYERS:
            raise ValueError(f"mlp_desc: network {i} has {len(layers)} layers (1..{MLP_MAX_LAYERS})")
        net = d.nets[i]
        net.n_layers = len(layers)
        net.dims[0] = int(layers[0][0].shape[1])
        for l, (w, b) in enumerate(layers):
            if w.dim() != 2 or w.shape[1] != net.dims[l] or b.shape != (w.shape[0],):
                raise ValueError(f"mlp_desc: network {i} layer {l}: weight {tuple(w.shape)}, bias {tuple(b.shape)}")
            net.dims[l + 1] = int(w.shape[0])
            net.W[l], net.b[l] = w.data_ptr(), b.data_ptr()
    return d


def mlp_packed_bytes(desc: MlpDesc) -> int:
    lib = learn_library()
    nbytes = lib.h12learn_mlp_packed_bytes(C.byref(desc))
    if nbytes == 0:
        _check(lib, -1, "h12learn_mlp_packed_bytes")
    return nbytes


def mlp_pack(desc: MlpDesc, packed: torch.Tensor):
    """Re-packs the weights ``desc`` points to into ``packed`` (one launch on the current stream)."""
    lib = learn_library()
    _f32(packed, "packed")
    if packed.numel() * 4 < mlp_packed_bytes(desc):
        raise ValueError("mlp_pack: packed is smaller than mlp_packed_bytes(desc)")
    _check(lib, lib.h12learn_mlp_pack(C.byref(desc), packed.data_ptr(), _stream(packed.device)), "h12learn_mlp_pack")


def mlp_forward(desc: MlpDesc, packed: torch.Tensor, x: torch.Tensor, out=None) -> tuple:
    """One launch: the outputs ([n][d_out] each) of every network of ``desc`` on ``x`` [n][d_in]."""
    lib = learn_library()
    _f32(packed, "packed"), _f32(x, "x")
    if x.dim() != 2 or x.shape[1] != desc.d_in or x.shape[0] < 1:
        raise ValueError(f"mlp_forward: x {tuple(x.shape)} is not (n >= 1, {desc.d_in})")
    n = x.shape[0]
    widths = [desc.nets[i].dims[desc.nets[i].n_layers] for i in range(desc.n_nets)]
    if out is None:
        out = tuple(torch.empty((n, w), dtype=torch.float32, device=x.device) for w in widths)
    for i, (y, w) in enumerate(zip(out, widths)):
        if _f32(y, f"out[{i}]").shape != (n, w):
            raise ValueError(f"mlp_forward: out[{i}] must be ({n}, {w})")
    ys = (C.c_void_p * desc.n_nets)(*[y.data_ptr() for y in out])
    _check(lib, lib.h12learn_mlp_forward(C.byref(desc), packed.data_ptr(), x.data_ptr(), n, ys, _stream(x.device)),
           "h12learn_mlp_forward")
    return tuple(out)


# ---- training side of the fused MLP (csrc/h12_policy_train.hip): one network, no normaliser
def mlp_train_rows() -> int:
    return learn_library().h12learn_mlp_train_rows()


def mlp_train_max_width() -> int:
    return learn_library().h12learn_mlp_train_max_width()


def mlp_packed_t_bytes(desc: MlpDesc) -> int:
    lib = learn_library()
    nbytes = lib.h12learn_mlp_packed_t_bytes(C.byref(desc))
    if nbytes == 0:
        _check(lib, -1, "h12learn_mlp_packed_t_bytes")
    return nbytes


def mlp_pack_t(desc: MlpDesc, packed_t: torch.Tensor):
    """Packs the transposed weights of ``desc`` (the dgrad's operand) into ``packed_t``: one launch."""
    lib = learn_library()
    _f32(packed_t, "packed_t")
    if packed_t.numel() * 4 < mlp_packed_t_bytes(desc):
        raise ValueError("mlp_pack_t: packed_t is smaller than mlp_packed_t_bytes(desc)")
    _check(lib, lib.h12learn_mlp_pack_t(C.byref(desc), packed_t.data_ptr(), _stream(packed_t.device)),
           "h12learn_mlp_pack_t")


def _widths(desc: MlpDesc) -> list[int]:
    net = desc.nets[0]
    return [net.dims[l] for l in range(net.n_layers + 1)]


def mlp_forward_train(desc: MlpDesc, packed: torch.Tensor, x: torch.Tensor):
    """One launch: (y [n][d_out], [h_l [n][dims[l+1]] for every hidden layer]) of the one network of ``desc``."""
    lib = learn_library()
    _f32(packed, "packed"), _f32(x, "x")
    dims = _widths(desc)
    if x.dim() != 2 or x.shape[1] != dims[0] or x.shape[0] < 1:
        raise ValueError(f"mlp_forward_train: x {tuple(x.shape)} is not (n >= 1, {dims[0]})")
    n = x.shape[0]
    y = torch.empty((n, dims[-1]), dtype=torch.float32, device=x.device)
    hs = [torch.empty((n, w), dtype=torch.float32, device=x.device) for w in dims[1:-1]]
    hp = (C.c_void_p * max(1, len(hs)))(*[h.data_ptr() for h in hs])
    _check(lib, lib.h12learn_mlp_forward_train(C.byref(desc), packed.data_ptr(), x.data_ptr(), n, y.data_ptr(), hp,
                                               _stream(x.device)), "h12learn_mlp_forward_train")
    return y, hs


def mlp_backward(desc: MlpDesc, packed_t: torch.Tensor, dy: torch.Tensor, hs, need_dx: bool = False):
    """Two launches: ([dZ_l for every hidden layer], [db_l for every layer], dX or None) from ``dy`` [n][d_out], the
    activations ``hs`` saved by mlp_forward_train and the transposed pack."""
    lib = learn_library()
    _f32(packed_t, "packed_t"), _f32(dy, "dy")
    dims = _widths(desc)
    if dy.dim() != 2 or dy.shape[1] != dims[-1] or dy.shape[0] < 1:
        raise ValueError(f"mlp_backward: dy {tuple(dy.shape)} is not (n >= 1, {dims[-1]})")
    n, dev = dy.shape[0], dy.device
    if len(hs) != len(dims) - 2:
        raise ValueError(f"mlp_backward: {len(hs)} saved activations for {len(dims) - 2} hidden layers")
    for l, h in enumerate(hs):
        if _f32(h, f"hs[{l}]").shape != (n, dims[l + 1]):
            raise ValueError(f"mlp_backward: hs[{l}] must be ({n}, {dims[l + 1]})")
    dzs = [torch.empty((n, w), dtype=torch.float32, device=dev) for w in dims[1:-1]]
    dbs = [torch.empty(w, dtype=torch.float32, device=dev) for w in dims[1:]]
    dx = torch.empty((n, dims[0]), dtype=torch.float32, device=dev) if need_dx else None
    nbytes = lib.h12learn_mlp_backward_workspace_bytes(C.byref(desc), n)
    if nbytes == 0:
        _check(lib, -1, "h12learn_mlp_backward_workspace_bytes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    arr = lambda ts: (C.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])  # noqa: E731
    _check(lib, lib.h12learn_mlp_backward(C.byref(desc), packed_t.data_ptr(), dy.data_ptr(), arr(hs), n, arr(dzs),
                                          arr(dbs), None if dx is None else dx.data_ptr(), ws.data_ptr(), nbytes,
                                          _stream(dev)), "h12learn_mlp_backward")
    return dzs, dbs, dx


# ---- fused recurrent policy step (csrc/h12_policy_rnn.hip): LSTM cell + MLP of up to 2 networks over one input
def lstm_max_hidden() -> int:
    return learn_library().h12learn_lstm_max_hidden()


def lstm_desc(cells, nets, norm_kind: int = MLP_NORM_NONE, norm_mean: torch.Tensor | None = None,
              norm_scale: torch.Tensor | None = None, norm_eps: float = 0.0) -> LstmDesc:
    """The descriptor of ``cells``, a list of nn.LSTM layer-0 parameter tuples (weight_ih [4H][d_in], weight_hh [4H][H],
    bias_ih [4H], bias_hh [4H]), and ``nets``, the MLP after each cell as for mlp_desc.  Shapes and data pointers only;
    the caller keeps the tensors alive and in place."""
    if not 1 <= len(cells) <= LSTM_MAX_NETS or len(nets) != len(cells):
        raise ValueError(f"lstm_desc: {len(cells)} cells and {len(nets)} networks (1..{LSTM_MAX_NETS} of each)")
    d = LstmDesc()
    four_h, d.d_in = (int(v) for v in cells[0][0].shape)
    d.hidden = four_h // 4
    d.norm_kind, d.norm_eps = int(norm_kind), float(norm_eps)
    if norm_kind != MLP_NORM_NONE:
        d.norm_mean, d.norm_scale = norm_mean.data_ptr(), norm_scale.data_ptr()
    for i, (w_ih, w_hh, b_ih, b_hh) in enumerate(cells):
        if (w_ih.shape != (four_h, d.d_in) or w_hh.shape != (four_h, d.hidden) or b_ih.shape != (four_h,)
                or b_hh.shape != (four_h,) or four_h != 4 * d.hidden):
            raise ValueError(f"lstm_desc: cell {i}: weight_ih {tuple(w_ih.shape)}, weight_hh {tuple(w_hh.shape)}, biases "
                             f"{tuple(b_ih.shape)}, {tuple(b_hh.shape)}")
        c = d.cells[i]
        c.w_ih, c.w_hh, c.b_ih, c.b_hh = w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr()
    d.mlp = mlp_desc(nets)
    return d


def lstm_packed_bytes(desc: LstmDesc) -> int:
    lib = learn_library()
    nbytes = lib.h12learn_lstm_packed_bytes(C.byref(desc))
    if nbytes == 0:
        _check(lib, -1, "h12learn_lstm_packed_bytes")
    return nbytes


def lstm_pack(desc: LstmDesc, packed: torch.Tensor):
    """Re-packs the parameters ``desc`` points to into ``packed`` (one launch on the current stream)."""
    lib = learn_library()
    _f32(packed, "packed")
    if packed.numel() * 4 < lstm_packed_bytes(desc):
        raise ValueError("lstm_pack: packed is smaller than lstm_packed_bytes(desc)")
    _check(lib, lib.h12learn_lstm_pack(C.byref(desc), packed.data_ptr(), _stream(packed.device)), "h12learn_lstm_pack")


def lstm_step(desc: LstmDesc, packed: torch.Tensor, x: torch.Tensor, states, reset: torch.Tensor | None = None,
              out_states=None, out=None) -> tuple:
    """One launch: every network of ``desc`` steps once on ``x`` [n][d_in].  ``states``: per network (h, c), [n][H] each,
    updated IN PLACE unless ``out_states`` (the same layout) is given.  ``reset``: None, or n uint8 / bool entries; a
    non-zero entry makes that row read h = c = 0.  Returns the networks' outputs ([n][d_out] each)."""
    lib = learn_library()
    _f32(packed, "packed"), _f32(x, "x")
    nn_ = desc.mlp.n_nets
    if x.dim() != 2 or x.shape[1] != desc.d_in or x.shape[0] < 1:
        raise ValueError(f"lstm_step: x {tuple(x.shape)} is not (n >= 1, {desc.d_in})")
    n = x.shape[0]
    if out_states is None:
        out_states = states
    if len(states) != nn_ or len(out_states) != nn_:
        raise ValueError(f"lstm_step: {len(states)} states for {nn_} networks")
    for i, pair in enumerate(list(states) + list(out_states)):
        for t in pair:
            if _f32(t, f"states[{i % nn_}]").shape != (n, desc.hidden):
                raise ValueError(f"lstm_step: every state tensor must be ({n}, {desc.hidden}), got {tuple(t.shape)}")
    widths = [desc.mlp.nets[i].dims[desc.mlp.nets[i].n_layers] for i in range(nn_)]
    if out is None:
        out = tuple(torch.empty((n, w), dtype=torch.float32, device=x.device) for w in widths)
    for i, (y, w) in enumerate(zip(out, widths)):
        if _f32(y, f"out[{i}]").shape != (n, w):
            raise ValueError(f"lstm_step: out[{i}] must be ({n}, {w})")
    io = LstmIo()
    io.x, io.n = x.data_ptr(), n
    if reset is not None:
        if not (reset.is_cuda and reset.dtype in (torch.uint8, torch.bool) and reset.is_contiguous()
                and reset.numel() == n):
            raise ValueError(f"lstm_step: reset must be a contiguous uint8 or bool CUDA tensor of {n} entries")
        io.reset = reset.data_ptr()
    for i in range(nn_):
        io.h_in[i], io.c_in[i] = states[i][0].data_ptr(), states[i][1].data_ptr()
        io.h_out[i], io.c_out[i] = out_states[i][0].data_ptr(), out_states[i][1].data_ptr()
        io.y[i] = out[i].data_ptr()
    _check(lib, lib.h12learn_lstm_step(C.byref(desc), packed.data_ptr(), C.byref(io), _stream(x.device)),
           "h12learn_lstm_step")
    return tuple(out)


# ---- the recurrent policy's update (csrc/h12_policy_rnn_train.hip): LSTM over [T][n] with done resets, and its BPTT
def lstm_seq_desc(w_hhs) -> LstmSeqDesc:
    """The descriptor of the weight_hh [4H][H] tensors of 1..2 networks of one hidden size.  Shapes and data pointers
    only; the caller keeps the tensors alive and in place."""
    if not 1 <= len(w_hhs) <= LSTM_MAX_NETS:
        raise ValueError(f"lstm_seq_desc: {len(w_hhs)} networks (1..{LSTM_MAX_NETS})")
    d = LstmSeqDesc()
    d.n_nets, d.hidden = len(w_hhs), int(w_hhs[0].shape[1])
    for i, w in enumerate(w_hhs):
        if _f32(w, f"w_hh[{i}]").shape != (4 * d.hidden, d.hidden):
            raise ValueError(f"lstm_seq_desc: w_hh[{i}] {tuple(w.shape)} is not ({4 * d.hidden}, {d.hidden})")
        d.w_hh[i] = w.data_ptr()
    return d


def lstm_seq_packed_bytes(desc: LstmSeqDesc) -> int:
    lib = learn_library()
    nbytes = lib.h12learn_lstm_seq_packed_bytes(C.byref(desc))
    if nbytes == 0:
        _check(lib, -1, "h12learn_lstm_seq_packed_bytes")
    return nbytes


def lstm_seq_pack(desc: LstmSeqDesc, packed: torch.Tensor) -> torch.Tensor:
    """One launch: W_hh and W_hh^T of every network of ``desc`` into ``packed`` (lstm_seq_packed_bytes)."""
    lib = learn_library()
    nbytes = lstm_seq_packed_bytes(desc)
    if _f32(packed, "packed").numel() * 4 < nbytes:
        raise ValueError("lstm_seq_pack: packed is smaller than lstm_seq_packed_bytes(desc)")
    _check(lib, lib.h12learn_lstm_seq_pack(C.byref(desc), packed.data_ptr(), _stream(packed.device)),
           "h12learn_lstm_seq_pack")
    return packed


def _seq_dones(dones: torch.Tensor, T: int, n: int, fn: str):
    if not (dones.is_cuda and dones.dtype in (torch.uint8, torch.bool) and dones.is_contiguous()
            and dones.shape == (T, n)):
        raise ValueError(f"{fn}: dones must be a contiguous uint8 or bool CUDA tensor of ({T}, {n})")
    return dones


def _seq_same(ts, shape, name: str, fn: str):
    for i, t in enumerate(ts):
        if _f32(t, f"{name}[{i}]").shape != shape:
            raise ValueError(f"{fn}: {name}[{i}] {tuple(t.shape)} is not {tuple(shape)}")


def lstm_seq_forward(desc: LstmSeqDesc, packed: torch.Tensor, zxs, dones: torch.Tensor, h0s, c0s, out=None):
    """One launch: per network (h_seq [T][n][H], c_seq [T][n][H], gates [T][n][4H]) from the input projections ``zxs``
    ([T][n][4H] each), ``dones`` ([T][n] bytes) and the t = 0 states ``h0s`` / ``c0s`` ([n][H] each).  ``out``: the same
    triples preallocated."""
    lib = learn_library()
    _f32(packed, "packed")
    nn_, H = desc.n_nets, desc.hidden
    if not (len(zxs) == len(h0s) == len(c0s) == nn_) or zxs[0].dim() != 3:
        raise ValueError(f"lstm_seq_forward: {len(zxs)} projections, {len(h0s)} / {len(c0s)} states for {nn_} networks")
    T, n = int(zxs[0].shape[0]), int(zxs[0].shape[1])
    _seq_same(zxs, (T, n, 4 * H), "zxs", "lstm_seq_forward")
    _seq_same(list(h0s) + list(c0s), (n, H), "states", "lstm_seq_forward")
    _seq_dones(dones, T, n, "lstm_seq_forward")
    dev = zxs[0].device
    if out is None:
        out = [tuple(torch.empty((T, n, w), dtype=torch.float32, device=dev) for w in (H, H, 4 * H))
               for _ in range(nn_)]
    io = LstmSeqIo()
    io.T, io.n, io.dones = T, n, dones.data_ptr()
    for i in range(nn_):
        _seq_same(out[i][:2], (T, n, H), "out", "lstm_seq_forward")
        _seq_same(out[i][2:], (T, n, 4 * H), "out", "lstm_seq_forward")
        io.zx[i], io.h0[i], io.c0[i] = zxs[i].data_ptr(), h0s[i].data_ptr(), c0s[i].data_ptr()
        io.h_seq[i], io.c_seq[i], io.gates[i] = (t.data_ptr() for t in out[i])
    _check(lib, lib.h12learn_lstm_seq_forward(C.byref(desc), packed.data_ptr(), C.byref(io), _stream(dev)),
           "h12learn_lstm_seq_forward")
    return out


def lstm_seq_backward(desc: LstmSeqDesc, packed: torch.Tensor, dh_seqs, saved, dones: torch.Tensor, c0s,
                      need_state_grads: bool = True, out=None):
    """One launch: per network (dz [T][n][4H], dh0 [n][H] or None, dc0 [n][H] or None) from ``dh_seqs`` ([T][n][H]
    each) and ``saved``, per network the (c_seq, gates) of lstm_seq_forward.  ``out``: the same triples preallocated."""
    lib = learn_library()
    _f32(packed, "packed")
    nn_, H = desc.n_nets, desc.hidden
    if not (len(dh_seqs) == len(saved) == len(c0s) == nn_) or dh_seqs[0].dim() != 3:
        raise ValueError(f"lstm_seq_backward: {len(dh_seqs)} gradients, {len(saved)} saved for {nn_} networks")
    T, n = int(dh_seqs[0].shape[0]), int(dh_seqs[0].shape[1])
    _seq_same(dh_seqs, (T, n, H), "dh_seqs", "lstm_seq_backward")
    _seq_same([s[0] for s in saved], (T, n, H), "c_seq", "lstm_seq_backward")
    _seq_same([s[1] for s in saved], (T, n, 4 * H), "gates", "lstm_seq_backward")
    _seq_same(c0s, (n, H), "c0s", "lstm_seq_backward")
    _seq_dones(dones, T, n, "lstm_seq_backward")
    dev = dh_seqs[0].device
    if out is None:
        out = [(torch.empty((T, n, 4 * H), dtype=torch.float32, device=dev),
                torch.empty((n, H), dtype=torch.float32, device=dev) if need_state_grads else None,
                torch.empty((n, H), dtype=torch.float32, device=dev) if need_state_grads else None)
               for _ in range(nn_)]
    io = LstmSeqGradIo()
    io.T, io.n, io.dones = T, n, dones.data_ptr()
    for i in range(nn_):
        dz, dh0, dc0 = out[i]
        _seq_same([dz], (T, n, 4 * H), "dz", "lstm_seq_backward")
        _seq_same([t for t in (dh0, dc0) if t is not None], (n, H), "dh0 / dc0", "lstm_seq_backward")
        io.dh_seq[i], io.c_seq[i], io.gates[i] = dh_seqs[i].data_ptr(), saved[i][0].data_ptr(), saved[i][1].data_ptr()
        io.c0[i], io.dz[i] = c0s[i].data_ptr(), dz.data_ptr()
        io.dh0[i] = None if dh0 is None else dh0.data_ptr()
        io.dc0[i] = None if dc0 is None else dc0.data_ptr()
    _check(lib, lib.h12learn_lstm_seq_backward(C.byref(desc), packed.data_ptr(), C.byref(io), _stream(dev)),
           "h12learn_lstm_seq_backward")
    return out


# ---- fused loss heads (csrc/h12_ppo_head.hip): what ppo_head and cleanrl_head check and allocate alike
def _head_check(head: str, mean, value, param, param_name: str, per_row, idx, idx_rows, stats_accum, n_stats: int):
    """The networks' outputs (mean [m][A], value of m elements, the std parameter of A), the per-row rollout tensors
    (name, tensor; n_src elements each), idx (None, or ``idx_rows`` int64 entries; None: m) and stats_accum (None, or at
    least n_stats floats).  Returns (m, A, n_src)."""
    _f32(mean, "mean"), _f32(value, "value"), _f32(param, param_name)
    if mean.dim() != 2 or mean.shape[0] < 1 or mean.shape[1] < 1:
        raise ValueError(f"{head}: mean {tuple(mean.shape)} is not (m >= 1, A >= 1)")
    m, A = mean.shape
    if value.numel() != m or param.numel() != A:
        raise ValueError(f"{head}: value has {value.numel()} and {param_name} {param.numel()} elements for mean "
                         f"{tuple(mean.shape)}")
    n_src = per_row[0][1].numel()
    for name, t in per_row:
        if _f32(t, name).numel() != n_src:
            raise ValueError(f"{head}: {name} must have {n_src} elements")
    rows = m if idx_rows is None else idx_rows
    if idx is not None and not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous()
                                and idx.shape == (rows,)):
        raise ValueError(f"{head}: idx must be a contiguous int64 CUDA tensor of {rows} entries")
    if stats_accum is not None and _f32(stats_accum, "stats_accum").numel() < n_stats:
        raise ValueError(f"{head}: stats_accum must have at least {n_stats} elements")
    return m, A, n_src


def _head_outputs(m: int, A: int, dev):
    """(d_mean [m][A], d_value [m], the std parameter's gradient [A], out [5]), uninitialised."""
    return (torch.empty((m, A), dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.float32, device=dev),
            torch.empty(A, dtype=torch.float32, device=dev), torch.empty(5, dtype=torch.float32, device=dev))


def _head_fill(a, mean, value, idx, old_log_prob, advantages, actions, outputs, stats_accum, ws, nbytes: int):
    """The fields the two argument structs name alike (the std parameter and its gradient are set by the caller)."""
    a.m, a.A = mean.shape
    a.n_src = old_log_prob.numel()
    a.mean, a.value = mean.data_ptr(), value.data_ptr()
    a.idx = None if idx is None else idx.data_ptr()
    a.old_log_prob, a.advantages, a.actions = old_log_prob.data_ptr(), advantages.data_ptr(), actions.data_ptr()
    a.d_mean, a.d_value, a.out = outputs[0].data_ptr(), outputs[1].data_ptr(), outputs[3].data_ptr()
    a.stats_accum = None if stats_accum is None else stats_accum.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes


def ppo_head_rows() -> int:
    return learn_library().h12learn_ppo_head_rows()


def ppo_head_max_actions() -> int:
    return learn_library().h12learn_ppo_head_max_actions()


def ppo_head(mean: torch.Tensor, value: torch.Tensor, std_param: torch.Tensor, std_kind: int, idx, n_rows: int,
             old_log_prob, advantages, returns, target_values, old_mu, old_sigma, actions, actions_direct: bool,
             clip_param: float, value_loss_coef: float, entropy_coef: float, use_clipped_value_loss: bool,
             lr: torch.Tensor | None = None, desired_kl: float | None = None, stats_accum: torch.Tensor | None = None):
    """Two launches: (d_mean [m][A], d_value [m], d_param [A], out [5]) of the PPO loss head on mean [m][A], value
    (m elements) and the std parameter [A].  ``n_rows`` is B, the minibatch's rows (m, or m / 2 under augmentation);
    idx (None, or B int64 entries) selects the rows of the rollout tensors (n_src rows each; actions [m][A] with
    ``actions_direct``).  ``lr`` (a device scalar; needs desired_kl) and ``stats_accum`` (3 floats) are updated in place
    when given.  include/h12learn.h has the formulae."""
    lib = learn_library()
    B = int(n_rows)
    m, A, n_src = _head_check("ppo_head", mean, value, std_param, "std_param",
                              (("old_log_prob", old_log_prob), ("advantages", advantages), ("returns", returns),
                               ("target_values", target_values)), idx, B, stats_accum, 3)
    for name, t in (("old_mu", old_mu), ("old_sigma", old_sigma)):
        if _f32(t, name).shape != (n_src, A):
            raise ValueError(f"ppo_head: {name} must be ({n_src}, {A})")
    if _f32(actions, "actions").shape != ((m, A) if actions_direct else (n_src, A)):
        raise ValueError(f"ppo_head: actions {tuple(actions.shape)} for m = {m}, n_src = {n_src}, "
                         f"actions_direct = {bool(actions_direct)}")
    if lr is not None and (_f32(lr, "lr").numel() != 1 or desired_kl is None):
        raise ValueError("ppo_head: lr must be one float32 element and needs desired_kl")
    nbytes = lib.h12learn_ppo_head_workspace_bytes(m, A)
    if nbytes == 0:
        _check(lib, -1, "h12learn_ppo_head_workspace_bytes")
    outputs = _head_outputs(m, A, mean.device)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=mean.device)  # a fresh one per call
    a = PpoHeadArgs()
    _head_fill(a, mean, value, idx, old_log_prob, advantages, actions, outputs, stats_accum, ws, nbytes)
    a.B, a.std_kind, a.actions_direct = B, int(std_kind), int(bool(actions_direct))
    a.use_clipped_value_loss = int(bool(use_clipped_value_loss))
    a.std_param, a.d_param = std_param.data_ptr(), outputs[2].data_ptr()
    a.returns, a.target_values = returns.data_ptr(), target_values.data_ptr()
    a.old_mu, a.old_sigma = old_mu.data_ptr(), old_sigma.data_ptr()
    a.clip_param, a.value_loss_coef, a.entropy_coef = float(clip_param), float(value_loss_coef), float(entropy_coef)
    a.desired_kl = 0.0 if desired_kl is None else float(desired_kl)
    a.lr = None if lr is None else lr.data_ptr()
    _check(lib, lib.h12learn_ppo_head(C.byref(a), _stream(mean.device)), "h12learn_ppo_head")
    return outputs


def cleanrl_head_rows() -> int:
    return learn_library().h12learn_cleanrl_head_rows()


_cleanrl_ws: dict = {}


def cleanrl_head_workspace(m: int, A: int, device) -> torch.Tensor:
    """The head's workspace for [m][A] outputs, cached per (device, m, A); it needs no initialisation and is reused by
    every call of that shape (calls on one stream are ordered, and the head reads only what it has just written)."""
    key = (torch.device(device), int(m), int(A))
    ws = _cleanrl_ws.get(key)
    if ws is None:
        lib = learn_library()
        nbytes = lib.h12learn_cleanrl_head_workspace_bytes(m, A)
        if nbytes == 0:
            _check(lib, -1, "h12learn_cleanrl_head_workspace_bytes")
        ws = _cleanrl_ws[key] = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    return ws


def cleanrl_head(mean: torch.Tensor, value: torch.Tensor, logstd: torch.Tensor, idx, old_log_prob, advantages,
                 returns_n, values_n, actions, value_mean: torch.Tensor, value_var: torch.Tensor, value_eps: float,
                 clip_coef: float, ent_coef: float, vf_coef: float, norm_adv: bool, clip_vloss: bool,
                 stats_accum: torch.Tensor | None = None, workspace: torch.Tensor | None = None):
    """Three launches: (d_mean [m][A], d_value [m], d_logstd [A], out [5]) of the CleanRL loss head on mean [m][A],
    value (m elements) and actor_logstd (A elements).  idx (None, or m int64 entries) selects the rows of the rollout
    tensors (n_src rows each); value_mean / value_var are value_rms's device scalars, read by the kernel.
    ``stats_accum`` (5 floats) is updated in place when given; ``workspace`` defaults to the cached one.
    include/h12learn.h has the formulae."""
    lib = learn_library()
    m, A, n_src = _head_check("cleanrl_head", mean, value, logstd, "logstd",
                              (("old_log_prob", old_log_prob), ("advantages", advantages), ("returns_n", returns_n),
                               ("values_n", values_n)), idx, None, stats_accum, 5)
    if _f32(actions, "actions").shape != (n_src, A):
        raise ValueError(f"cleanrl_head: actions {tuple(actions.shape)} must be ({n_src}, {A})")
    for name, t in (("value_mean", value_mean), ("value_var", value_var)):
        if _f32(t, name).numel() != 1:
            raise ValueError(f"cleanrl_head: {name} must be one float32 element")
    ws = cleanrl_head_workspace(m, A, mean.device) if workspace is None else workspace
    if not (ws.is_cuda and ws.is_contiguous()):
        raise ValueError("cleanrl_head: workspace must be a contiguous CUDA tensor")
    outputs = _head_outputs(m, A, mean.device)
    a = CleanRlHeadArgs()
    _head_fill(a, mean, value, idx, old_log_prob, advantages, actions, outputs, stats_accum, ws,
               ws.numel() * ws.element_size())
    a.norm_adv, a.clip_vloss = int(bool(norm_adv)), int(bool(clip_vloss))
    a.logstd, a.d_logstd = logstd.data_ptr(), outputs[2].data_ptr()
    a.returns_n, a.values_n = returns_n.data_ptr(), values_n.data_ptr()
    a.value_mean, a.value_var, a.value_eps = value_mean.data_ptr(), value_var.data_ptr(), float(value_eps)
    a.clip_coef, a.ent_coef, a.vf_coef = float(clip_coef), float(ent_coef), float(vf_coef)
    _check(lib, lib.h12learn_cleanrl_head(C.byref(a), _stream(mean.device)), "h12learn_cleanrl_head")
    return outputs


# ---- Random Network Distillation's reward step (csrc/h12_rnd.hip)
def rnd_reward(desc: MlpDesc, packed: torch.Tensor, x: torch.Tensor, err: torch.Tensor | None = None,
               xn: torch.Tensor | None = None, emb: bool = False):
    """One launch: err [n] = the row norm of target - predictor on the normalised ``x`` [n][d_in] (desc: nets[0] the
    predictor, nets[1] the target).  ``xn`` ([n][d_in] or None) receives the normalised rows.  Returns err, or with
    ``emb`` (a test hook) (err, predictor embedding, target embedding)."""
    lib = learn_library()
    _f32(packed, "packed"), _f32(x, "x")
    if x.dim() != 2 or x.shape[1] != desc.d_in or x.shape[0] < 1:
        raise ValueError(f"rnd_reward: x {tuple(x.shape)} is not (n >= 1, {desc.d_in})")
    n = x.shape[0]
    if err is None:
        err = torch.empty(n, dtype=torch.float32, device=x.device)
    elif _f32(err, "err").shape != (n,):
        raise ValueError(f"rnd_reward: err must be ({n},)")
    if xn is not None and _f32(xn, "xn").shape != x.shape:
        raise ValueError("rnd_reward: xn must have x's shape")
    embs, ptrs = None, None
    if emb:
        w = desc.nets[0].dims[desc.nets[0].n_layers]
        embs = tuple(torch.empty((n, w), dtype=torch.float32, device=x.device) for _ in range(2))
        ptrs = (C.c_void_p * 2)(*[e.data_ptr() for e in embs])
    _check(lib, lib.h12learn_rnd_reward(C.byref(desc), packed.data_ptr(), x.data_ptr(), n, err.data_ptr(),
                                        None if xn is None else xn.data_ptr(), ptrs, _stream(x.device)),
           "h12learn_rnd_reward")
    return (err, *embs) if emb else err


def rnd_finish(args: RndFinishArgs, device):
    """One launch of one block: reward normaliser, weight and the sum with the env's reward (h12learn_rnd_finish).  The
    caller fills ``args`` with the data pointers of tensors it keeps alive."""
    lib = learn_library()
    _check(lib, lib.h12learn_rnd_finish(C.byref(args), _stream(device)), "h12learn_rnd_finish")


# ---- fused optimiser step (csrc/h12_optim.hip): gradient clip + Adam / RAdam of every tensor in two launches
def optim_chunk() -> int:
    return learn_library().h12learn_optim_chunk()


def optim_max_tensors() -> int:
    return learn_library().h12learn_optim_max_tensors()


def optim_fold() -> int:
    return learn_library().h12learn_optim_fold()


def optim_workspace_bytes(numels) -> int:
    lib = learn_library()
    numels = [int(n) for n in numels]
    nbytes = lib.h12learn_optim_workspace_bytes((C.c_longlong * max(1, len(numels)))(*numels), len(numels))
    if nbytes == 0:
        _check(lib, -1, "h12learn_optim_workspace_bytes")
    return nbytes


def optim_step(rule: int, params, grads, exp_avgs, exp_avg_sqs, steps, beta1: float, beta2: float, eps: float,
               max_norm: float | None, lr, workspace: torch.Tensor, grad_norm: torch.Tensor | None = None):
    """Two launches (h12learn_optim_step): the global norm of ``grads``, then the clip coefficient and the Adam
    (OPTIM_ADAM) or RAdam (OPTIM_RADAM) update of every tensor of ``params`` with its moments, in place.  ``steps``: one
    float32 device scalar per tensor, incremented by the call.  ``lr``: a float, or a float32 device scalar the kernel
    reads.  ``max_norm``: None or <= 0 for no clip.  ``grad_norm`` (a float32 device scalar) receives the norm.
    ``workspace``: at least optim_workspace_bytes of the tensors' sizes.  The gradients are not rescaled in memory."""
    lib = learn_library()
    n = len(params)
    if not (n >= 1 and len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(steps) == n):
        raise ValueError(f"optim_step: {n} parameters, {len(grads)} gradients, {len(exp_avgs)} / {len(exp_avg_sqs)} "
                         f"moments, {len(steps)} steps")
    for i in range(n):
        numel = params[i].numel()
        for name, t in (("params", params[i]), ("grads", grads[i]), ("exp_avgs", exp_avgs[i]),
                        ("exp_avg_sqs", exp_avg_sqs[i])):
            if _f32(t, f"{name}[{i}]").numel() != numel or numel < 1:
                raise ValueError(f"optim_step: {name}[{i}] has {t.numel()} elements, params[{i}] {numel} (>= 1)")
        if _f32(steps[i], f"steps[{i}]").numel() != 1:
            raise ValueError(f"optim_step: steps[{i}] must be one float32 element")
    if not (workspace.is_cuda and workspace.is_contiguous()):
        raise ValueError("optim_step: workspace must be a contiguous CUDA tensor")
    a = OptimArgs()
    a.rule, a.n_tensors = int(rule), n
    a.beta1, a.beta2, a.eps = float(beta1), float(beta2), float(eps)
    a.max_norm = 0.0 if max_norm is None else float(max_norm)
    if torch.is_tensor(lr):
        if _f32(lr, "lr").numel() != 1:
            raise ValueError("optim_step: a tensor lr must be one float32 element")
        a.lr, a.lr_dev = 0.0, lr.data_ptr()
    else:
        a.lr = float(lr)
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    a.p, a.g, a.exp_avg, a.exp_avg_sq, a.step = ptrs(params), ptrs(grads), ptrs(exp_avgs), ptrs(exp_avg_sqs), ptrs(steps)
    a.numel = (C.c_longlong * n)(*[p.numel() for p in params])
    if grad_norm is not None:
        if _f32(grad_norm, "grad_norm").numel() != 1:
            raise ValueError("optim_step: grad_norm must be one float32 element")
        a.grad_norm = grad_norm.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    _check(lib, lib.h12learn_optim_step(C.byref(a), _stream(params[0].device)), "h12learn_optim_step")
