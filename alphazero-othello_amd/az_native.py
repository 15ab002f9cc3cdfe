"""ctypes binding of the C-ABI library `libaz_othello.so` (include/az_othello.h).

The whole product path goes through this module: the OthelloGameNew drop-in
(envs/othello.py), the MCTS drop-in (MCTS_model.py) and the batched self-play engine
(engine.py).  There is no fallback: if the library is missing this module raises on
import, naming the build command.

Error mapping follows the reference's Python conventions:
AZ_ERR_ILLEGAL -> ValueError("Illegal move: a") (envs/othello.py:421),
AZ_ERR_STATE -> KeyError(action) (MCTS_model.py:214), everything else -> RuntimeError.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# AZ_LIB_PATH: an alternative build of the same library (experiment builds, scripts/exp)
LIB_PATH = os.environ.get("AZ_LIB_PATH") or os.path.join(HERE, "libaz_othello.so")

AZ_OK = 0
AZ_ERR_ILLEGAL = -1
AZ_ERR_ARG = -2
AZ_ERR_HIP = -3
AZ_ERR_CAPACITY = -4
AZ_ERR_STATE = -5

AZ_FLAG_TERMINAL = 1
AZ_FLAG_NOPLACE = 2
AZ_FLAG_ILLEGAL = 4
AZ_FLAG_PASSED = 8

AZ_SOLVE_SKIPPED, AZ_SOLVE_ABORTED, AZ_SOLVE_MAX_EMPTIES = -128, -127, 14
AZ_SOLVE_DEEP_MAX_EMPTIES = 20
AZ_SEARCH_SKIPPED, AZ_SEARCH_ABORTED, AZ_SEARCH_MAX_DEPTH = -32768, -32767, 10
AZ_REC_TERMINAL, AZ_REC_UNFINISHED, AZ_REC_ILLEGAL, AZ_REC_OVERFLOW = 0, 1, 2, 3
AZ_REC_PASS_ROWS, AZ_REC_MAX_STRIDE, AZ_REC_MAX_ROWS = 1, 128, 128
AZ_CANON_BAD = 255

AZ_EVAL_EXTERNAL, AZ_EVAL_ROLLOUT = 0, 1
AZ_RNG_DEVICE, AZ_RNG_INJECTED = 0, 1
AZ_GAME_IDLE, AZ_GAME_ACTIVE, AZ_GAME_FINISHED, AZ_GAME_SEARCH_DONE = 0, 1, 2, 3


class AzConfig(ctypes.Structure):
    _fields_ = [
        ("n_games", ctypes.c_int32),
        ("node_capacity", ctypes.c_int32),
        ("max_plies", ctypes.c_int32),
        ("num_simulations", ctypes.c_int32),
        ("c_puct", ctypes.c_double),
        ("dirichlet_alpha", ctypes.c_double),
        ("dirichlet_epsilon", ctypes.c_double),
        ("temperature", ctypes.c_double),
        ("num_exploratory_moves", ctypes.c_int32),
        ("lambd", ctypes.c_double),
        ("eval_mode", ctypes.c_int32),
        ("rng_mode", ctypes.c_int32),
        ("d4_augment", ctypes.c_int32),
        ("auto_play", ctypes.c_int32),
        ("refill", ctypes.c_int32),
        ("sample_capacity", ctypes.c_int64),
        ("inj_noise_slots", ctypes.c_int32),
        ("inj_uniform_slots", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("stream_id", ctypes.c_uint64),
        ("leaves_per_step", ctypes.c_int32),
    ]


_P = ctypes.c_void_p
_I = ctypes.c_int
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_U32 = ctypes.c_uint32
_U64 = ctypes.c_uint64
_D = ctypes.c_double

AZ_CONV_SPLIT3, AZ_CONV_FP16, AZ_CONV_FP16X2 = 0, 1, 2  # conv kernel numerics modes

# name -> argtypes (restype is int for every entry point except az_last_error)
SIGNATURES = {
    "az_abi_version": [],
    "oth_legal_cpu": [_P, _P, _P, _I64],
    "oth_step_cpu": [_P, _P, _P, _P, _P, _P, _P, _I64],
    "oth_make_move_cpu": [_P, _P, _P, _P, _P, _I64],
    "oth_pack_np": [_P, _P, _P, _P, _I64],
    "oth_unpack_np": [_P, _P, _P, _P, _I64],
    "oth_d4_cpu": [_P, _P, _P, _I64],
    "oth_legal_gpu": [_P, _P, _P, _I64, _P],
    "oth_step_gpu": [_P, _P, _P, _P, _P, _P, _P, _I64, _P],
    "oth_d4_gpu": [_P, _P, _P, _I64, _P],
    "oth_step_io_gpu": [_P, _P, _P, _P, _P, _P, _P, _I64, _P],
    "az_engine_create": [ctypes.POINTER(AzConfig), ctypes.POINTER(_P)],
    "az_engine_destroy": [_P],
    "az_engine_geometry": [_P, _P, _P, _P],
    "az_reset_all": [_P, _I64, _I32, _P],
    "az_set_root": [_P, _I32, _U64, _U64, _I32, _P],
    "az_begin_search": [_P, _I32, _I32, _P],
    "az_select": [_P, _P, _P, _P],
    "az_expand_backup": [_P, _P, _P, _P],
    "az_play": [_P, _P],
    "az_engine_defer_moves": [_P, _I32],
    "az_engine_set_stem": [_P, _P, _P, _P, _P, _I32],
    "az_select_move": [_P, _P, _P, _I32, _P],
    "az_select_move_expand": [_P, _P, _P, _P, _P, _I32, _P],
    "az_select_expand": [_P, _P, _P, _P, _P, _P],
    "az_expand_backup_par": [_P, _P, _P, _I32, _P],
    "az_move_flush": [_P, _I32, _P],
    "az_inject": [_P, _P, _P, _P],
    "az_root_policy": [_P, _I32, _D, _D, _P, _P, _P, _P],
    "az_make_move": [_P, _I32, _I32, _P],
    "az_counters": [_P, _P, _P],
    "az_set_roots": [_P, _P, _P, _P, _P, _I32, _P],
    "az_begin_search_slots": [_P, _P, _I32, _I32, _P],
    "az_root_stats": [_P, _P, _P, _P],
    "az_reroot_slots": [_P, _P, _P, _P],
    "az_game_info": [_P, _P, _P, _P, _P, _P, _P, _P],
    "az_export_tree": [_P, _I32, _I32] + [_P] * 14,
    "az_export_trajectory": [_P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P],
    "az_samples": [_P, _P, _P, _P, _P, _P, _P, _P],
    "az_copy_samples": [_P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P],
    "az_clear_samples": [_P, _P],
    "az_bias_act_gpu": [_P, _P, _P, _I64, _I32, _I32, _P],
    "az_conv3x3_gpu": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _P],
    "az_conv_stem_gpu": [_P, _P, _P, _P, _I32, _I32, _P],
    "az_conv_stem2_gpu": [_P, _P, _P, _P, _I32, _I32, _P, _P],
    "az_conv3x3_cfg_gpu": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P],
    "az_conv3x3_mx_prep_gpu": [_P, _P, _I32, _I32, _P],
    "az_conv3x3_mx_prep_bytes": [_I32, _I32],
    "az_heads_fast_gemm_gpu": [_P, _P, _P, _I32, _P, _I32, _I32, _I32, _I32, _P],
    "az_fast_trunk_gpu": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P],
    "az_conv3x3_mx_gpu": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P],
    "az_conv3x3_wino_prep_gpu": [_P, _P, _I32, _I32, _P],
    "az_conv3x3_wino_gpu": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P],
    "az_conv3x3_wino4_gpu": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P],
    "az_conv3x3_wino4_splitk_gpu": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P,
                                    _I32, _P],
    "az_conv3x3_wino4_heads_gpu": [_P, _P, _P, _P, _I32, _I32, _I32] + [_P] * 11 + [_P],
    "az_board_absmax_gpu": [_P, _I32, _I32, _P, _P],
    "az_conv3x3_wino_prep_bytes": [_I32, _I32],
    "az_trunk_wino_gpu": [_P] * 7 + [_I32] * 4 + [_P],
    "az_trunk_wino4_gpu": [_P] * 11 + [_I32] * 3 + [_P],
    "az_trunk_wino4_heads_gpu": [_P] * 11 + [_I32] * 3 + [_P] * 10 + [_P],
    "az_trunk_wino4_heads_fp16_gpu": [_P] * 11 + [_I32] * 3 + [_P] * 10 + [_P],
    "az_heads_az_gpu": [_P] * 11 + [_I32, _I32, _P],
    "az_heads_fast_finish_gpu": [_P, _I32, _I32, _P, _P, _P, _P, _P, _I32, _P],
    "az_conv3x3_mx_cfg_gpu": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P],
    "az_conv3x3_mx_stem_gpu": [_P] * 7 + [_I32, _I32, _I32, _I32, _P],
    "az_replay_aggregate_gpu": [_P] * 5 + [_I64] + [_P] * 10,
    "oth_solve_cpu": [_P, _P, _I64, _I32, _U64, _P, _P, _P],
    "oth_solve_gpu": [_P, _P, _I64, _I32, _U64, _I32, _P, _P, _P, _P, _P, _P],
    "oth_solve_deep_cpu": [_P, _P, _I64, _I32, _I32, _I32, _U64, _P, _P, _P],
    "oth_solve_deep_gpu": [_P, _P, _I64, _I32, _I32, _I32, _U64, _I32, _P, _P, _P, _P, _P, _P],
    "oth_solve_moves_cpu": [_P, _P, _I64, _I32, _I32, _U64, _P, _P, _P],
    "oth_line_step_cpu": [_P, _P, _P, _P, _I64, _I32, _I32] + [_P] * 9,
    "oth_line_step_gpu": [_P, _P, _P, _P, _I64, _I32, _I32] + [_P] * 9 + [_P],
    "az_leaf_solve_cpu": [_P, _P, _I64, _I32, _U64, _P],
    "az_leaf_solve_gpu": [_P, _P, _I64, _I32, _U64, _P, _P, _P],
    "az_leaf_solve_stats_gpu": [_P, _P, _P],
    "oth_eval_cpu": [_P, _P, _I64, _P],
    "oth_eval_gpu": [_P, _P, _I64, _P, _P],
    "oth_search_cpu": [_P, _P, _I64, _I32, _U64, _P, _P, _P],
    "oth_search_gpu": [_P, _P, _I64, _I32, _U64, _I32, _P, _P, _P, _P, _P, _P],
    "oth_records_cpu": [_P, _I32, _P, _P, _P, _I64, _I32, _I32] + [_P] * 12,
    "oth_records_gpu": [_P, _I32, _P, _P, _P, _I64, _I32, _I32] + [_P] * 12 + [_P],
    "az_records_vote_gpu": [_P] * 4 + [_I64] + [_P] * 9,
    "oth_canon_cpu": [_P, _P, _I64, _P, _P, _P, _P],
    "oth_canon_gpu": [_P, _P, _I64, _P, _P, _P, _P, _P],
    "az_copy16_probe_gpu": [_P, _P, _I64, _P],
    "az_rows_d4_cpu": [_P, _P, _P, _P, _I64, _P, _P],
    "az_rows_d4_gpu": [_P, _P, _P, _P, _I64, _P, _P, _P],
    "az_rows_symmetrise_cpu": [_P, _P, _I64, _P],
    "az_rows_symmetrise_gpu": [_P, _P, _I64, _P, _P],
    "az_rng_uniform_cpu": [_U64, _U32, _U32, _I64, _U32, _U32, _P],
    "az_rng_uniform_gpu": [_U64, _U32, _U32, _I64, _U32, _U32, _P, _P],
    "az_rng_dirichlet_gpu": [_U64, _U32, _U32, _I64, _U32, _D, _P, _P, _P],
}


def _load():
    # torch ships its own HIP runtime and preloads it by path; loading ours first would put
    # a second copy of libamdhip64 / libhsa-runtime64 in the process (the second HSA
    # instance then sees no device).  With torch loaded first, the library's
    # libamdhip64.so.7 dependency resolves to torch's copy by soname: one runtime.
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (build()) "
            "or `python alphazero-othello_amd/az_build.py`; there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("az_last_error", "az_build_id"):
        getattr(lib, name).argtypes = []
        getattr(lib, name).restype = ctypes.c_char_p
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _I
    lib.az_conv3x3_wino_prep_bytes.restype = _I64
    lib.az_conv3x3_mx_prep_bytes.restype = _I64
    return lib


lib = _load()


def build_id():
    """sha256 of the sources the loaded library was compiled from (az_build.source_hash)."""
    return lib.az_build_id().decode()


def last_error():
    m = lib.az_last_error()
    return m.decode() if m else ""


def check(rc, what=""):
    """Raise the reference's exception type for a failed C-ABI call."""
    if rc == AZ_OK:
        return
    msg = last_error()
    if rc == AZ_ERR_ILLEGAL:
        raise ValueError(msg or f"Illegal move ({what})")
    if rc == AZ_ERR_STATE:
        try:
            key = int(msg.split(":")[0])
        except ValueError:
            key = msg
        raise KeyError(key)
    raise RuntimeError(f"{what} failed ({rc}): {msg}")


def ptr(a):
    """Host numpy array or device torch tensor -> void*."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"], "buffer must be C-contiguous"
        return a.ctypes.data_as(_P)
    return _P(a.data_ptr())  # torch tensor


def stream_ptr(stream=None):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return _P(s.cuda_stream)


# ---- thin typed wrappers over the stateless CPU board entry points ----------------------

def _u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def legal_cpu(own, opp):
    own, opp = _u64(own), _u64(opp)
    out = np.empty(own.shape, np.uint64)
    check(lib.oth_legal_cpu(ptr(own), ptr(opp), ptr(out), own.size), "oth_legal_cpu")
    return out


def step_cpu(own, opp, act, raise_illegal=True):
    own, opp = _u64(own), _u64(opp)
    act = np.ascontiguousarray(act, dtype=np.uint8)
    n = own.size
    o, p, lg = (np.empty(own.shape, np.uint64) for _ in range(3))
    st = np.empty(own.shape, np.uint16)
    rc = lib.oth_step_cpu(ptr(own), ptr(opp), ptr(act), ptr(o), ptr(p), ptr(lg), ptr(st), n)
    if rc != AZ_OK and (raise_illegal or rc != AZ_ERR_ILLEGAL):
        check(rc, "oth_step_cpu")
    return o, p, lg, st


def make_move_cpu(own, opp, act):
    own, opp = _u64(own), _u64(opp)
    act = np.ascontiguousarray(act, dtype=np.uint8)
    o, p = np.empty(own.shape, np.uint64), np.empty(own.shape, np.uint64)
    check(lib.oth_make_move_cpu(ptr(own), ptr(opp), ptr(act), ptr(o), ptr(p), own.size),
          "oth_make_move_cpu")
    return o, p


def pack_np(states, player):
    states = np.ascontiguousarray(states, dtype=np.int8).reshape(-1, 64)
    player = np.ascontiguousarray(np.broadcast_to(player, (states.shape[0],)), dtype=np.int8)
    n = states.shape[0]
    own, opp = np.empty(n, np.uint64), np.empty(n, np.uint64)
    check(lib.oth_pack_np(ptr(states), ptr(player), ptr(own), ptr(opp), n), "oth_pack_np")
    return own, opp


def unpack_np(own, opp, player):
    own, opp = _u64(own).reshape(-1), _u64(opp).reshape(-1)
    n = own.size
    player = np.ascontiguousarray(np.broadcast_to(player, (n,)), dtype=np.int8)
    out = np.empty((n, 64), np.int8)
    check(lib.oth_unpack_np(ptr(own), ptr(opp), ptr(player), ptr(out), n), "oth_unpack_np")
    return out.reshape(n, 8, 8)


def d4_cpu(x, sym):
    x = _u64(x)
    sym = np.ascontiguousarray(np.broadcast_to(sym, x.shape), dtype=np.uint8)
    out = np.empty(x.shape, np.uint64)
    check(lib.oth_d4_cpu(ptr(x), ptr(sym), ptr(out), x.size), "oth_d4_cpu")
    return out


def solve_cpu(own, opp, max_empties=12, node_limit=1 << 31):
    """Exact endgame solve on the host: (score int8, best uint8, nodes uint64) per position
    (AZ_SOLVE_SKIPPED / AZ_SOLVE_ABORTED in score for positions not solved)."""
    own, opp = _u64(own), _u64(opp)
    score = np.empty(own.shape, np.int8)
    best = np.empty(own.shape, np.uint8)
    nodes = np.empty(own.shape, np.uint64)
    check(lib.oth_solve_cpu(ptr(own), ptr(opp), own.size, int(max_empties), int(node_limit),
                            ptr(score), ptr(best), ptr(nodes)), "oth_solve_cpu")
    return score, best, nodes


def solve_deep_cpu(own, opp, max_empties=16, alpha=-65, beta=65, node_limit=1 << 31):
    """Windowed, move-ordered endgame solve on the host (up to AZ_SOLVE_DEEP_MAX_EMPTIES
    empties): (score int8, best uint8, nodes uint64) per position; score is exact inside
    (alpha, beta) and a bound on the true score outside it."""
    own, opp = _u64(own), _u64(opp)
    score = np.empty(own.shape, np.int8)
    best = np.empty(own.shape, np.uint8)
    nodes = np.empty(own.shape, np.uint64)
    check(lib.oth_solve_deep_cpu(ptr(own), ptr(opp), own.size, int(max_empties), int(alpha),
                                 int(beta), int(node_limit), ptr(score), ptr(best), ptr(nodes)),
          "oth_solve_deep_cpu")
    return score, best, nodes


def solve_deep_gpu(own, opp, max_empties=16, alpha=-65, beta=65, node_limit=1 << 31,
                   split_plies=0, stream=None):
    """oth_solve_deep_gpu on int64 device tensors (the uint64 bitboards' bits), asynchronous
    on `stream` (default: the current stream).  Returns device tensors (score int8, best
    uint8, nodes int64 = the uint64 counts' bits)."""
    import torch

    dev = own.device
    n = own.numel()
    score = torch.empty(n, dtype=torch.int8, device=dev)
    best = torch.empty(n, dtype=torch.uint8, device=dev)
    nodes = torch.empty(n, dtype=torch.int64, device=dev)
    need = ctypes.c_size_t(0)
    args = (int(max_empties), int(alpha), int(beta), int(node_limit), int(split_plies))
    check(lib.oth_solve_deep_gpu(None, None, n, *args, None, None, None, None,
                                 ctypes.byref(need), None), "oth_solve_deep_gpu")
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
            check(lib.oth_solve_deep_gpu(ptr(own), ptr(opp), n, *args, ptr(score), ptr(best),
                                         ptr(nodes), ptr(ws), ctypes.byref(need),
                                         stream_ptr(s)), "oth_solve_deep_gpu")
    return score, best, nodes


AZ_MOVES_NONE = -128
AZ_MOVES_SCORES, AZ_MOVES_WLD, AZ_MOVES_OPTIMAL = 0, 1, 2


def solve_moves_cpu(own, opp, max_empties=12, mode=AZ_MOVES_SCORES, node_limit=1 << 31):
    """The exact value of every move on the host: (values int8 [n, 65] with AZ_MOVES_NONE
    where the action is not available, score int8, nodes uint64) per root; see
    include/az_othello.h for the three modes."""
    own, opp = _u64(own).reshape(-1), _u64(opp).reshape(-1)
    values = np.empty((own.size, 65), np.int8)
    score = np.empty(own.size, np.int8)
    nodes = np.empty(own.size, np.uint64)
    check(lib.oth_solve_moves_cpu(ptr(own), ptr(opp), own.size, int(max_empties), int(mode),
                                  int(node_limit), ptr(values), ptr(score), ptr(nodes)),
          "oth_solve_moves_cpu")
    return values, score, nodes


AZ_LEAF_SOLVE_MAX_EMPTIES = 12
LEAF_SOLVE_STATS = ("solved", "limited", "nodes")


def leaf_solve_cpu(nn_in, values, max_empties, node_limit):
    """az_leaf_solve_cpu on host arrays: `values` (float32 [rows], C-contiguous) is updated
    in place from the planes nn_in (float32 [rows, 64]); returns this call's counters."""
    nn_in = np.ascontiguousarray(nn_in, np.float32)
    assert values.dtype == np.float32 and values.flags["C_CONTIGUOUS"]
    rows = values.size
    assert nn_in.size == rows * 64
    stats = np.zeros(3, np.uint64)
    check(lib.az_leaf_solve_cpu(ptr(nn_in), ptr(values), rows, int(max_empties),
                                int(node_limit), ptr(stats)), "az_leaf_solve_cpu")
    return dict(zip(LEAF_SOLVE_STATS, (int(x) for x in stats)))


def leaf_solve_workspace(rows, device):
    """A zeroed workspace for az_leaf_solve_gpu calls of up to `rows` rows (one owner, one
    stream)."""
    import torch

    need = ctypes.c_size_t(0)
    check(lib.az_leaf_solve_gpu(None, None, int(rows), 1, 1, None, ctypes.byref(need), None),
          "az_leaf_solve_gpu")
    return torch.zeros(need.value // 8, dtype=torch.int64, device=device)


def leaf_solve_gpu(nn_in, values, max_empties, node_limit, workspace, stream=None):
    """az_leaf_solve_gpu on device tensors (row slices of larger buffers are fine),
    asynchronous on `stream` (default: the current stream); `values` is updated in place."""
    import torch

    rows = values.numel()
    assert nn_in.dtype == values.dtype == torch.float32
    assert nn_in.is_contiguous() and values.is_contiguous() and nn_in.numel() == rows * 64
    have = ctypes.c_size_t(workspace.numel() * workspace.element_size())
    with torch.cuda.device(values.device):
        check(lib.az_leaf_solve_gpu(ptr(nn_in), ptr(values), rows, int(max_empties),
                                    int(node_limit), ptr(workspace), ctypes.byref(have),
                                    stream_ptr(stream)), "az_leaf_solve_gpu")


def leaf_solve_stats_gpu(workspace, stream=None):
    """The counters accumulated in a workspace (synchronises `stream`)."""
    import torch

    stats = np.zeros(3, np.uint64)
    with torch.cuda.device(workspace.device):
        check(lib.az_leaf_solve_stats_gpu(ptr(workspace), ptr(stats), stream_ptr(stream)),
              "az_leaf_solve_stats_gpu")
    return dict(zip(LEAF_SOLVE_STATS, (int(x) for x in stats)))


def eval_cpu(own, opp):
    """Heuristic evaluation on the host: int16 per position (T(d) for terminal positions)."""
    own, opp = _u64(own), _u64(opp)
    value = np.empty(own.shape, np.int16)
    check(lib.oth_eval_cpu(ptr(own), ptr(opp), own.size, ptr(value)), "oth_eval_cpu")
    return value


def search_cpu(own, opp, depth, node_limit=1 << 31):
    """Depth-limited alpha-beta on the host: (value int16, best uint8, nodes uint64) per
    position (AZ_SEARCH_SKIPPED / AZ_SEARCH_ABORTED in value for positions not searched)."""
    own, opp = _u64(own), _u64(opp)
    value = np.empty(own.shape, np.int16)
    best = np.empty(own.shape, np.uint8)
    nodes = np.empty(own.shape, np.uint64)
    check(lib.oth_search_cpu(ptr(own), ptr(opp), own.size, int(depth), int(node_limit),
                             ptr(value), ptr(best), ptr(nodes)), "oth_search_cpu")
    return value, best, nodes


# ---- test support: the engine's device random draws as arrays (csrc/rng_probe.hip) --------

def rng_uniform_cpu(seed, stream_id, slot0, n, event, sub):
    """azr::uniform2 on the host for slots slot0 .. slot0 + n - 1: double [n, 2]."""
    out = np.empty((int(n), 2), np.float64)
    check(lib.az_rng_uniform_cpu(int(seed), int(stream_id), int(slot0), int(n), int(event),
                                 int(sub), ptr(out)), "az_rng_uniform_cpu")
    return out


def rng_uniform_gpu(seed, stream_id, slot0, n, event, sub, device="cuda"):
    """The same draws from the device: a float64 device tensor [n, 2]."""
    import torch

    out = torch.empty((int(n), 2), dtype=torch.float64, device=device)
    with torch.cuda.device(out.device):
        check(lib.az_rng_uniform_gpu(int(seed), int(stream_id), int(slot0), int(n), int(event),
                                     int(sub), ptr(out), stream_ptr()), "az_rng_uniform_gpu")
    return out


def rng_dirichlet_gpu(seed, stream_id, slot0, n, event, alpha, device="cuda"):
    """A root expansion's noise draw per slot: float64 device tensors (gammas [n, 65] raw,
    noise [n, 65] normalised)."""
    import torch

    gammas = torch.empty((int(n), 65), dtype=torch.float64, device=device)
    noise = torch.empty_like(gammas)
    with torch.cuda.device(gammas.device):
        check(lib.az_rng_dirichlet_gpu(int(seed), int(stream_id), int(slot0), int(n), int(event),
                                       float(alpha), ptr(gammas), ptr(noise), stream_ptr()),
              "az_rng_dirichlet_gpu")
    return gammas, noise


def status_flags(st):
    return np.asarray(st) & 0xFF


def status_score(st):
    return (np.asarray(st) >> 8).astype(np.uint8).view(np.int8).astype(np.int32)
