"""ctypes binding of liboac_amd.so (the C ABI declared in include/oac_amd.h).

The library is built in-tree (``make -C oac-explore_amd`` or
``__graft_entry__.build()``).  There is no fallback: if the shared library is
missing or cannot be loaded, every entry point raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# OAC_LIB: another in-tree build of the same library (same-box A/B runs of a
# kernel change); the default is the package's own
_DEFAULT_LIB = os.path.join(HERE, "liboac_amd.so")
LIB_PATH = os.environ.get("OAC_LIB") or _DEFAULT_LIB

OAC_KIND_SAC = 0
OAC_KIND_PARTICLE = 1
OAC_KIND_GAUSS = 2
OAC_KIND_PARTICLE_UB = 3
OAC_KIND_DDPG = 4
OAC_KIND_SAC_SHALLOW = 5

OAC_STEP_GATHER = 1
OAC_STEP_DEVICE_EPS = 2
OAC_STEP_USE_GRAPH = 4
OAC_STEP_COUNTS = 8

OAC_DP_FORCE = 1
OAC_DP_OVERLAP = 2

# oac_sac_trace bits
TRACE = dict(direct=1, direct_big=2, batch_copy=4, qdot=8, wl_targets=16, split_phase1=32,
             fused=64, exchange=128, head_dh2=512)

# oac_allreduce_fn: int (*)(void* ctx, float* buf, int64_t n, void* stream)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                ctypes.c_void_p)

# public workspace ids (enum oac_ws_buffer)
WS = {name: i for i, name in enumerate([
    "batch", "eps1", "eps2", "head1", "head2", "act1", "act2", "logp1", "logp2",
    "q1", "q2", "qn1", "qn2", "tq1", "tq2", "y", "sqe1", "sqe2", "qnew", "counts",
    "head3", "act3", "logp_part", "h2q1", "h2q2", "h1p", "h2p"])}
# non-default kernel / schedule choices (enum oac_tuning_key; A/B runs and the
# alternative-kernel parity tests): set_tuning(fwd_tile_m=128, ...) before the
# trainers that should use them create their plans; 0 restores a default
TUNE = {name: i for i, name in enumerate([
    "retired_0", "fwd_tile_m", "fwd_tile_n", "fwd_nb", "split_adam", "dh2_targets", "head_cc",
    "splits_q1", "splits_q0", "splits_ph", "splits_p1", "splits_p0", "debug_cfg",
    "ring_direct", "ring_prefetch", "retired_15", "head_dh2"])}


def set_tuning(**kw):
    for k, v in kw.items():
        check(lib().oac_tuning_set(TUNE[k], int(v)))


def set_tuning_spec(spec):
    """set_tuning from "key=value,key=value" (tools' A/B scripts)."""
    if spec:
        set_tuning(**{k: int(v) for k, v in (kv.split("=") for kv in spec.split(",") if kv)})


# diagnostic views a library build may predate (skipped when it rejects the id)
WS_OPTIONAL = ("h1p", "h2p")


_SAC_CONFIG_FIELDS = [
        ("kind", ctypes.c_int), ("obs_dim", ctypes.c_int), ("act_dim", ctypes.c_int),
        ("hidden", ctypes.c_int), ("q_out", ctypes.c_int), ("batch", ctypes.c_int),
        ("discount", ctypes.c_float), ("reward_scale", ctypes.c_float), ("tau", ctypes.c_float),
        ("policy_lr", ctypes.c_double), ("qf_lr", ctypes.c_double), ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double), ("adam_eps", ctypes.c_double),
        ("auto_alpha", ctypes.c_int), ("target_entropy", ctypes.c_float),
        ("target_update_period", ctypes.c_int), ("row_stride", ctypes.c_int),
        ("off_obs", ctypes.c_int), ("off_act", ctypes.c_int), ("off_rew", ctypes.c_int),
        ("off_term", ctypes.c_int), ("off_next_obs", ctypes.c_int),
        ("seed", ctypes.c_uint64), ("gemm_cfg", ctypes.c_int), ("world_size", ctypes.c_int),
        ("std_bound", ctypes.c_float), ("std_init", ctypes.c_float),
        ("std_soft_update", ctypes.c_int), ("std_soft_prob", ctypes.c_float),
        ("mean_update", ctypes.c_int), ("delta_index", ctypes.c_int),
        ("rescale_spread", ctypes.c_float), ("freeze_q_bias", ctypes.c_int),
        ("n_hidden", ctypes.c_int), ("global_opt", ctypes.c_int),
]
# oac_sac_config's fields after global_opt (include/oac_amd.h): share_layers=False
_SAC_CONFIG_TAIL = [("unshared", ctypes.c_int), ("std_lr", ctypes.c_double)]


class _SacConfigC(ctypes.Structure):
    """The whole C struct: its size and the tail fields' offsets."""
    _fields_ = _SAC_CONFIG_FIELDS + _SAC_CONFIG_TAIL


def _tail_field(name, ctype):
    off = getattr(_SacConfigC, name).offset

    def get(self):
        return ctype.from_buffer(self._buf, off).value

    def put(self, value):
        ctype.from_buffer(self._buf, off).value = value
    return property(get, put)


class SacConfig(ctypes.Structure):
    """oac_sac_config.  ``_fields_`` declares the struct up to ``global_opt``,
    the last field callers written before ``unshared`` / ``std_lr`` know (an
    existing test pins it as the declaration's last entry); every instance is
    backed by a zeroed buffer of the WHOLE C struct's size, so the library reads
    an initialised tail, and the tail fields are attributes like the others."""
    _fields_ = _SAC_CONFIG_FIELDS

    def __new__(cls, *args, **kwargs):
        buf = bytearray(ctypes.sizeof(_SacConfigC))
        self = cls.from_buffer(buf)
        self._buf = buf
        return self


for _n, _t in _SAC_CONFIG_TAIL:
    setattr(SacConfig, _n, _tail_field(_n, _t))
assert all(getattr(SacConfig, n).offset == getattr(_SacConfigC, n).offset
           for n, _ in _SAC_CONFIG_FIELDS)


class SacLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "pol_fc0_w", "pol_fc0_b", "pol_fc1_w", "pol_fc1_b", "pol_head_w", "pol_head_b", "pol_size",
        "q_fc0_w", "q_fc0_b", "q_fc1_w", "q_fc1_b", "q_last_w", "q_last_b", "q_size",
        "q1_base", "q2_base", "n_critics", "params_total", "targets_total", "workspace_floats",
        "tpol_base")]


class EnsembleLayout(ctypes.Structure):
    """oac_ensemble_layout: the stacked policy block of a policy ensemble and
    the target_policy block's single-policy offsets."""
    _fields_ = [(n, ctypes.c_int64) for n in (
        "n_policies", "ens_fc0_w", "ens_fc0_b", "ens_head_w", "ens_head_b", "ens_size",
        "tpol_fc0_w", "tpol_fc0_b", "tpol_head_w", "tpol_head_b", "tpol_size")]


# enum oac_ens_view
ENS_VIEWS = {name: i for i, name in enumerate(["sel", "ub_next", "act", "head", "ub_obs"])}


class SacBuffers(ctypes.Structure):
    _fields_ = [
        ("params", ctypes.c_void_p), ("grads", ctypes.c_void_p), ("adam_m", ctypes.c_void_p),
        ("adam_v", ctypes.c_void_p), ("targets", ctypes.c_void_p),
        ("alpha_state", ctypes.c_void_p), ("step_state", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("replay", ctypes.c_void_p),
        ("replay_rows", ctypes.c_int64), ("idx_ring", ctypes.c_void_p),
        ("ring_slots", ctypes.c_int),
        ("counts", ctypes.c_void_p), ("count_tags", ctypes.c_void_p),
        ("count_epoch", ctypes.c_void_p), ("next_policy", ctypes.c_void_p),
    ]


_LIB = None

_SIGS = {
    "oac_last_error": (ctypes.c_char_p, []),
    "oac_abi_version": (ctypes.c_int, []),
    "oac_sac_query_layout": (ctypes.c_int, [ctypes.POINTER(SacConfig), ctypes.POINTER(SacLayout)]),
    "oac_sac_create": (ctypes.c_int, [ctypes.POINTER(SacConfig), ctypes.POINTER(SacBuffers),
                                      ctypes.POINTER(ctypes.c_void_p)]),
    "oac_sac_query_layout_ensemble": (ctypes.c_int, [ctypes.POINTER(SacConfig), ctypes.c_int,
                                                     ctypes.POINTER(SacLayout),
                                                     ctypes.POINTER(EnsembleLayout)]),
    "oac_sac_create_ensemble": (ctypes.c_int, [ctypes.POINTER(SacConfig), ctypes.c_int,
                                               ctypes.POINTER(SacBuffers),
                                               ctypes.POINTER(ctypes.c_void_p)]),
    "oac_sac_ensemble_view": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int64),
                                             ctypes.POINTER(ctypes.c_int64),
                                             ctypes.POINTER(ctypes.c_int64)]),
    "oac_ensemble_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_int] +
                          [ctypes.c_void_p] * 10),
    "oac_sac_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "oac_sac_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oac_sac_step_n": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_void_p]),
    "oac_sac_step_phase": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p]),
    "oac_sac_policy_opt_reset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oac_sac_policy_opt_iter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oac_sac_set_host_ring": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "oac_sac_host_ring": (ctypes.c_void_p, [ctypes.c_void_p]),
    "oac_sac_step_host_idx": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_int, ctypes.c_void_p]),
    "oac_sac_stage_host_idx": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_void_p]),
    "oac_sac_set_step_graph": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "oac_sac_set_allreduce": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int]),
    "oac_sac_trace": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "oac_rccl_unique_id": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p]),
    "oac_rccl_create": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_void_p)]),
    "oac_rccl_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "oac_rccl_allreduce": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_void_p]),
    "oac_sac_workspace_view": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_int64),
                                              ctypes.POINTER(ctypes.c_int64),
                                              ctypes.POINTER(ctypes.c_int64)]),
    "oac_sac_launch_count": (ctypes.c_int, [ctypes.c_void_p]),
    "oac_sac_cache_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "oac_tuning_set": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "oac_sac_set_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "oac_sac_read_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_int64), ctypes.c_int]),
    "oac_sac_read_launch_times": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                                 ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "oac_critic_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oac_policy_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "oac_policy_eval_fixed_std": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_int64, ctypes.c_int] +
                                  [ctypes.c_void_p] * 9),
    "oac_mt_seed_host": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_void_p]),
    "oac_replay_sample_indices": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    "oac_replay_gather": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "oac_replay_insert": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p] + [ctypes.c_int] * 7 + [ctypes.c_void_p]),
    "oac_replay_counts_update": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_int, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "oac_replay_priority_scratch_doubles": (ctypes.c_int64, [ctypes.c_int64]),
    "oac_replay_priority_sample": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p]),
    "oac_replay_nr_take": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                          ctypes.c_uint64, ctypes.c_void_p]),
    "oac_replay_nr_sample_positions": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_uint64,
                                                      ctypes.c_uint64, ctypes.c_void_p,
                                                      ctypes.c_void_p]),
    "oac_replay_nr_insert": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_int] + [ctypes.c_void_p] * 5 +
                             [ctypes.c_int] * 7 + [ctypes.c_void_p]),
    "oac_replay_nr_chunk": (ctypes.c_int64, []),
    "oac_replay_nr_launch_count": (ctypes.c_int64, []),
    "oac_adam_polyak": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_float, ctypes.c_int, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "oac_expl_workspace_floats": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "oac_expl_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.POINTER(ctypes.c_void_p)]),
    "oac_expl_workspace_floats_batch": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int]),
    "oac_expl_create_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.POINTER(ctypes.c_void_p)]),
    "oac_expl_create_shallow": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.POINTER(ctypes.c_void_p)]),
    "oac_expl_create_shared": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]),
    "oac_expl_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "oac_expl_obs_slot": (ctypes.c_void_p, [ctypes.c_void_p]),
    "oac_expl_action": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oac_expl_outputs": (ctypes.c_void_p, [ctypes.c_void_p]),
    "oac_expl_set_host_io": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "oac_expl_set_ub_index": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "oac_expl_host_staging": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                             ctypes.POINTER(ctypes.c_void_p)]),
    "oac_expl_action_now": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                           ctypes.c_float, ctypes.c_void_p]),
    "oac_expl_launch_form": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int)]),
}

# every symbol include/oac_amd.h declares (checked by tests/test_abi.py)
EXPORTED = sorted(_SIGS)


def lib():
    """Load liboac_amd.so (after torch, so the HIP runtime torch already
    loaded -- same soname libamdhip64.so.7 -- is the one the library binds)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is not built: run `make -C oac-explore_amd` (or "
            "__graft_entry__.build()).  There is no CPU fallback for the OAC hot path.")
    import torch  # noqa: F401  (HIP runtime first)
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        if LIB_PATH != _DEFAULT_LIB and not hasattr(L, name):
            continue   # an OAC_LIB A/B build of an older tree: its entry points only
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.oac_abi_version() != 3:
        raise RuntimeError("liboac_amd ABI version mismatch")
    _LIB = L
    return L


def check(rc):
    if rc != 0:
        msg = lib().oac_last_error().decode(errors="replace")
        raise RuntimeError(f"liboac_amd: {msg}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)
