"""CPU checks of the C-ABI boundary: the library loads and exports every
symbol include/oac_amd.h declares; host-side layout logic (no GPU compute)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "oac_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(oac_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from oac_amd import _lib
    L = _lib.lib()
    decl = declared_functions()
    assert decl, "no declarations parsed"
    missing = [f for f in decl if not hasattr(L, f)]
    assert not missing, missing
    # and the ctypes binding covers exactly the declared surface
    assert sorted(_lib.EXPORTED) == decl


def test_abi_version_and_error_channel():
    from oac_amd import _lib
    L = _lib.lib()
    assert L.oac_abi_version() == 3
    cfg = _lib.SacConfig()
    cfg.kind = 7
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) != 0
    assert b"kind" in L.oac_last_error()


@pytest.mark.parametrize("dims", [(376, 17, 256), (111, 8, 256), (1, 1, 256), (11, 3, 32)])
def test_param_layout_matches_reference_parameter_counts(dims):
    """Arena layout covers exactly the reference's parameter counts
    (Humanoid policy 171,042, each critic 166,913)."""
    from oac_amd import _lib, row_layout
    Do, Da, H = dims
    cfg = _lib.SacConfig()
    cfg.kind, cfg.obs_dim, cfg.act_dim, cfg.hidden, cfg.q_out, cfg.batch = 0, Do, Da, H, 1, 256
    for k, v in row_layout(Do, Da).items():
        setattr(cfg, k, v)
    cfg.gemm_cfg = -1
    cfg.world_size = 1
    lay = _lib.SacLayout()
    assert _lib.lib().oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) == 0
    n_pol = H * Do + H + H * H + H + 2 * (Da * H + Da)
    n_q = H * (Do + Da) + H + H * H + H + H + 1
    assert lay.pol_size >= n_pol and lay.pol_size - n_pol < 4 * 6
    assert lay.q_size >= n_q and lay.q_size - n_q < 4 * 6
    if dims == (376, 17, 256):
        assert n_pol == 171042 and n_q == 166913
    for f in ("pol_fc0_w", "pol_fc0_b", "pol_fc1_w", "pol_fc1_b", "pol_head_w", "pol_head_b",
              "q_fc0_w", "q_fc0_b", "q_fc1_w", "q_fc1_b", "q_last_w", "q_last_b", "q1_base",
              "q2_base"):
        assert getattr(lay, f) % 4 == 0, f
    assert lay.workspace_floats > 0


@pytest.mark.parametrize("kind,q_out", [(0, 1), (1, 10), (2, 2), (3, 10), (4, 1)])
def test_every_kind_has_a_layout_and_its_views_fit_the_workspace(kind, q_out):
    """The per-kind table behind the handle (csrc/plan_api.hip kind_ops): each
    trainer kind lays out a workspace, and every public view of a handle of
    that kind lies inside it.  Host-only: with null buffers create makes no
    GPU call."""
    from oac_amd import _lib, row_layout
    L = _lib.lib()
    cfg = _lib.SacConfig()
    cfg.kind, cfg.obs_dim, cfg.act_dim, cfg.hidden, cfg.q_out, cfg.batch = kind, 11, 3, 32, q_out, 40
    for k, v in row_layout(11, 3).items():
        setattr(cfg, k, v)
    cfg.gemm_cfg = -1
    cfg.world_size = 1
    lay = _lib.SacLayout()
    assert L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) == 0, L.oac_last_error()
    assert lay.n_critics == (2 if kind == 0 else 1) and lay.workspace_floats > 0
    h = ctypes.c_void_p()
    bufs = _lib.SacBuffers()
    assert L.oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h)) == 0, L.oac_last_error()
    try:
        off, rows, cols = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        for name, which in _lib.WS.items():
            assert L.oac_sac_workspace_view(h, which, ctypes.byref(off), ctypes.byref(rows),
                                            ctypes.byref(cols)) == 0, name
            assert off.value >= 0 and rows.value >= 0 and cols.value >= 0, name
            assert off.value + rows.value * cols.value <= lay.workspace_floats, name
        # the step's batch is a view of every layout
        L.oac_sac_workspace_view(h, _lib.WS["batch"], ctypes.byref(off), ctypes.byref(rows),
                                 ctypes.byref(cols))
        assert (rows.value, cols.value) == (40, cfg.row_stride)
    finally:
        assert L.oac_sac_destroy(h) == 0


@pytest.mark.parametrize("kind,q_out", [(0, 1), (1, 10), (2, 2), (3, 10), (4, 1)])
def test_two_hidden_layers_refuse_a_width_below_4_by_name(kind, q_out):
    """The policy head kernel (csrc/head.hip) reads the hidden activations as
    float4 columns clamped to hidden - 4: any width from 4 is served, a
    narrower one is refused when the layout is queried and when the plan is
    created, before any buffer is touched."""
    from oac_amd import _lib, row_layout
    L = _lib.lib()

    def cfg_for(H, n_hidden):
        cfg = _lib.SacConfig()
        cfg.kind, cfg.obs_dim, cfg.act_dim, cfg.hidden, cfg.q_out, cfg.batch = kind, 11, 3, H, q_out, 40
        for k, v in row_layout(11, 3).items():
            setattr(cfg, k, v)
        cfg.gemm_cfg, cfg.world_size, cfg.n_hidden = -1, 1, n_hidden
        return cfg

    for n_hidden in (0, 2):
        for H in (1, 2, 3):
            cfg, lay = cfg_for(H, n_hidden), _lib.SacLayout()
            assert L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) != 0, (H, n_hidden)
            msg = L.oac_last_error()
            for w in (b"n_hidden = 2", b"hidden must be at least 4", b"got %d" % H):
                assert w in msg, (w, msg)
            h, bufs = ctypes.c_void_p(), _lib.SacBuffers()
            assert L.oac_sac_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h)) != 0
            assert not h.value and b"at least 4" in L.oac_last_error()
        for H in (4, 5, 30, 513):   # every width from 4, ragged ones included
            cfg, lay = cfg_for(H, n_hidden), _lib.SacLayout()
            assert L.oac_sac_query_layout(ctypes.byref(cfg), ctypes.byref(lay)) == 0, L.oac_last_error()


def test_row_layout_keeps_critic_input_contiguous():
    from oac_amd import row_layout
    r = row_layout(376, 17)
    assert r["off_act"] == r["off_obs"] + 376
    assert r["row_stride"] % 4 == 0 and r["row_stride"] >= 2 * 376 + 17 + 2


def test_product_path_has_no_fallback(monkeypatch, tmp_path):
    """Without the HIP library every entry point raises (no CPU fallback), and
    the product package never imports the oracle (test infrastructure)."""
    from oac_amd import _lib
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "liboac_amd.so"))
    with pytest.raises(RuntimeError):
        _lib.lib()
    pkg = os.path.join(ROOT, "oac-explore_amd", "oac_amd")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
            assert "sac_oracle" not in src, f


def _header_enum(prefix, end):
    """The members of a C enum in include/oac_amd.h, in order (prefix-named)."""
    src = open(os.path.join(ROOT, "include", "oac_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(" + prefix + r"[A-Z0-9_]+)\b\s*(?:=\s*\d+)?\s*,", src)
    return [n for n in dict.fromkeys(names) if n != end]


def test_tuning_keys_match_the_header_and_reject_unknown():
    """oac_amd._lib.TUNE names every oac_tuning_key in the header's order;
    oac_tuning_set takes each key (0 = the default) and rejects one past the
    end with a message (host-only: no GPU call)."""
    from oac_amd import _lib
    keys = _header_enum("OAC_TUNE_", "OAC_TUNE_COUNT")
    assert keys and len(keys) == len(_lib.TUNE)
    py = sorted(_lib.TUNE, key=_lib.TUNE.get)
    assert [k.lower() for k in (n[len("OAC_TUNE_"):] for n in keys)] == py
    L = _lib.lib()
    for name in py:
        _lib.set_tuning(**{name: 0})
    assert L.oac_tuning_set(len(py), 1) != 0
    assert b"tuning key" in L.oac_last_error()


def test_retired_tuning_keys_are_refused_by_name():
    """The two retired keys (once the backward tile configuration and the
    last-arrival Adam) refuse a non-zero value with a message that names the
    removal, instead of ignoring an old caller's choice; 0 is accepted, so a
    loop that resets every key keeps working; one past the end is still
    rejected (host-only: no GPU call)."""
    from oac_amd import _lib
    L = _lib.lib()
    retired = [n for n in _header_enum("OAC_TUNE_", "OAC_TUNE_COUNT") if "RETIRED" in n]
    assert retired == ["OAC_TUNE_RETIRED_0", "OAC_TUNE_RETIRED_15"]
    for name in retired:
        key = _lib.TUNE[name[len("OAC_TUNE_"):].lower()]
        assert key == int(name.rsplit("_", 1)[1])
        for value in (9, 1, -1):
            assert L.oac_tuning_set(key, value) != 0, (name, value)
            msg = L.oac_last_error()
            assert name.encode() in msg and b"removed" in msg and b"one configuration" in msg, msg
        assert L.oac_tuning_set(key, 0) == 0, name
    assert L.oac_tuning_set(len(_lib.TUNE), 0) != 0
    assert b"unknown tuning key" in L.oac_last_error()


def test_trace_bits_match_the_header():
    """oac_amd._lib.TRACE carries every OAC_TRACE_* bit the header defines."""
    from oac_amd import _lib
    src = open(os.path.join(ROOT, "include", "oac_amd.h")).read()
    bits = {n[len("OAC_TRACE_"):].lower(): int(v)
            for n, v in re.findall(r"#define\s+(OAC_TRACE_[A-Z0-9_]+)\s+(\d+)", src)}
    assert bits == _lib.TRACE


def test_eval_entry_points_refuse_one_float_past_the_lds_limit_by_name():
    """oac_critic_eval / oac_policy_eval / oac_policy_eval_fixed_std admit
    exactly the dynamic LDS their launch requests (csrc/mlp_eval.hip
    mlp_eval_lds_bytes: critic (din + 4 H + Q + 4) floats, policy (Do + 2 H +
    3 Da + 4), fixed std 2 Da + 2 more) up to 160 KiB = 40,960 floats: dims at
    the limit pass (n = 0: no launch), one float more is refused with the
    named message before any launch (host-only: the buffers are never read)."""
    from oac_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nets = (ctypes.c_void_p * 2)(p, p)
    offs = (ctypes.c_int64 * 6)(0, 0, -1, 0, 0, 0)

    def critic(Do, n):
        return L.oac_critic_eval(nets, 1, offs, Do, 1, 10236, 1, p, Do, p, 1, n, p, p, None)

    def policy(Do, n):
        return L.oac_policy_eval(p, offs, Do, 1, 20000, p, Do, n, p, p, p, p, p, p, p, None)

    def fixed(Do, n):
        return L.oac_policy_eval_fixed_std(p, offs, Do, 1, 20000, p, Do, n, p, p, p, p, p, p, p, p,
                                           None)

    for call, Do, floats, name in ((critic, 10, 10 + 1 + 4 * 10236 + 1 + 4, b"critic eval"),
                                   (policy, 953, 953 + 2 * 20000 + 3 + 4, b"policy eval"),
                                   (fixed, 949, 949 + 2 * 20000 + 5 + 6, b"policy eval (fixed std)")):
        assert floats == 40960
        assert call(Do, 0) == 0, L.oac_last_error()
        assert call(Do + 1, 1) != 0
        assert name + b": dims exceed the workgroup's LDS" in L.oac_last_error()
