"""C-ABI library: loads without a GPU, exports every symbol include/tokenpacker.h declares, and
rejects bad descriptors before touching the device.  No compute calls here."""
import ctypes
import os
import re

import pytest

from tokenpacker_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "tokenpacker.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tp_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = _capi.load_library()
    declared = _header_symbols()
    assert set(declared) == set(_capi.EXPORTED_SYMBOLS), declared
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/tokenpacker.h but not exported"
    assert lib.tp_version() == _capi.TP_ABI_VERSION


def test_struct_layouts_match_header():
    # tp_desc: 6 x int32 + float + int32 + the tuning-context pointer; tp_weights: 23 pointers
    assert ctypes.sizeof(_capi.tp_desc) == 40
    assert ctypes.sizeof(_capi.tp_weights) == 23 * ctypes.sizeof(ctypes.c_void_p)
    assert len(_capi.WEIGHT_FIELDS) == 23
    assert ctypes.sizeof(_capi.tp_linear_args) == 8 * 4 + 3 * 8 + 6 * 8 + 2 * 4 + 8


def test_sizes_and_descriptor_validation():
    lib = _capi.load_library()
    d = _capi.make_desc(256, 24, 2, 4096, _capi.TP_BF16)
    packed = lib.tp_packed_weight_bytes(ctypes.byref(d))
    # 36,722,688 parameters in 2-byte elements, + fp32 biases/colsums + alignment, + the optional
    # out_proj∘mlp[0] fold (W_om [D,1024] fp16) and its pack-time scratch (Wout^T fp16, fp32 product [D,1024])
    # + the per-head transposes of the folded K in-projection the absorbed schedule reads (w_qt, 2 MiB)
    # + Wc = W'·W2 for k and v and W'q·Wq1 for q (the fused LayerNorm chains, 6 MiB)
    # + the centred chain weights (k, v, q, and the k one's per-head transposes: 8 MiB), the triangular factors R of the three
    #   centred layer-2 weights (6 MiB) and the fp64 scratch of their pack-time Householder QR (3 x [1024][1025] + vectors)
    fold = 4096 * 1024 * 2 + 1024 * 1024 * 2 + 4096 * 1024 * 4 + 1024 * 1024 * 2 + 3 * 1024 * 1024 * 2 + 1024 * 1024 * 2   # (+ w_qt_c)
    # + the rows of the centred V chain weight as K-tile pairs hi_t | lo_t ([1024][2048] fp16, 4 MiB: the absorbed schedule's per-head V GEMM
    #   contracts u against the weight AND its fp16 rounding residual, GemmArgs::a_k_dup; round 4: [hi | hi | lo], 6 MiB; since round 5 interleaved K-tile pairs [hi_t | lo_t], 4 MiB)
    fold += 7 * 1024 * 1024 * 2 + 3 * (1024 * 1025 * 8 + 16 * 1024 * 8 + 16 * 8) + 2 * 1024 * 1024 * 2
    assert 36_722_688 * 2 + fold <= packed < 36_722_688 * 2 + fold + 300_000
    ws = lib.tp_workspace_bytes(ctypes.byref(d))
    assert 1.0e9 < ws < 1.3e9            # schedule-aware: the s = 2 default writes neither H2 nor K | V nor Q1pre
    # bad scale factor: the reference's ValueError (builder.py:51-52)
    bad = _capi.make_desc(1, 24, 5, 4096, _capi.TP_BF16)
    assert lib.tp_workspace_bytes(ctypes.byref(bad)) == 0
    assert "scale_factor must be divisible by grid size" in _capi.last_error()
    with pytest.raises(ValueError, match="scale_factor must be divisible by grid size"):
        _capi.check(_capi.TP_ERR_BAD_SCALE, "x")
    for kw in (dict(batch=0), dict(hidden_size=100), dict(dtype=_capi.TP_F32), dict(out_dtype=7)):
        args = dict(batch=1, raw_grid=24, scale_factor=2, hidden_size=4096, dtype=_capi.TP_BF16)
        out_dtype = kw.pop("out_dtype", None)
        args.update(kw)
        dd = _capi.make_desc(args["batch"], args["raw_grid"], args["scale_factor"], args["hidden_size"],
                             args["dtype"], out_dtype)
        assert lib.tp_packed_weight_bytes(ctypes.byref(dd)) == 0, kw
        assert _capi.last_error()


def test_null_arguments_are_rejected_before_launch():
    lib = _capi.load_library()
    d = _capi.make_desc(1, 24, 2, 256, _capi.TP_BF16)
    st = _capi.strides3((576 * 1024, 1024, 1))
    rc = lib.tp_forward(ctypes.byref(d), None, st, None, st, None, None, None, 0, None)
    assert rc == _capi.TP_ERR_INVALID_ARG
    rc = lib.tp_pack_weights(ctypes.byref(d), None, None, 0, None)
    assert rc == _capi.TP_ERR_INVALID_ARG
    a = _capi.tp_linear_args()
    assert lib.tp_linear(ctypes.byref(a), None) == _capi.TP_ERR_INVALID_ARG
    assert lib.tp_set_tuning(99, 0) == _capi.TP_ERR_INVALID_ARG
    assert lib.tp_set_tuning(_capi.TP_TUNE_GEMM_TILE, 0) == _capi.TP_OK


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    monkeypatch.setattr(_capi, "_lib", None)
    with pytest.raises(_capi.TokenPackerLibraryError, match="no CPU fallback"):
        _capi.load_library(str(tmp_path / "libtokenpacker_hip.so"))


def test_train_hd_and_parts_entry_points_reject_bad_arguments():
    """The round's newer entry points validate before they touch the device, like tp_forward does."""
    lib = _capi.load_library()
    d = _capi.make_desc(1, 24, 2, 256, _capi.TP_BF16)
    st = _capi.strides3((576 * 1024, 1024, 1))
    E = _capi.TP_ERR_INVALID_ARG
    assert lib.tp_forward_train(ctypes.byref(d), None, st, None, st, None, None, None, 0, None) == E
    assert lib.tp_forward_parts(ctypes.byref(d), None, st, None, st, None, None, None, 0, None) == E
    assert lib.tp_forward_train_parts(ctypes.byref(d), None, st, None, st, None, None, None, 0, None) == E
    assert lib.tp_backward(ctypes.byref(d), None, st, None, None, None, None, None, None, 0, None) == E
    assert lib.tp_backward_parts(ctypes.byref(d), None, st, None, None, None, None, None, None, 0, None) == E
    assert _capi.last_error()
    # sizes: the training workspace extends the inference one by the two pre-GELU buffers and every slab the backward reads
    # (the inference one carries the K-split partials of a small batch, which the training forward never uses: compare without)
    _capi.set_tuning(_capi.TP_TUNE_SPLIT_K, 2)
    try:
        ws, tws, bws = (f(ctypes.byref(d)) for f in (lib.tp_workspace_bytes, lib.tp_train_workspace_bytes,
                                                     lib.tp_backward_workspace_bytes))
    finally:
        _capi.set_tuning(_capi.TP_TUNE_SPLIT_K, 0)
    assert 0 < ws < tws and bws > 0
    bad = _capi.make_desc(1, 24, 5, 256, _capi.TP_BF16)
    assert lib.tp_train_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.tp_backward_workspace_bytes(ctypes.byref(bad)) == 0
    # HD helpers
    assert lib.tp_hd_rows(1, 1, 144) == 145            # one crop: its tokens + '\n', no global view
    assert lib.tp_hd_rows(2, 3, 144) == (6 * 144 + 6) + 145
    assert lib.tp_hd_assemble(None, 1, None, 1, None, None, None, None, 145, 144, 256, _capi.TP_BF16, None) == E
    plan = (_capi.tp_hd_image * 1)(_capi.tp_hd_image(0, 1, 1, 0, 0))
    assert lib.tp_hd_assemble(plan, 0, None, 1, None, None, None, None, 145, 144, 256, _capi.TP_BF16, None) in (E, _capi.TP_OK)
    assert lib.tp_hd_assemble(plan, 1, None, 1, None, None, None, None, 145, 144, 256, _capi.TP_BF16, None) == E
    # plan validation (host-side, before anything is enqueued): overlap, out-of-order, reads / writes past the buffers
    fake = ctypes.c_void_p(4096)                                   # non-NULL, 16-byte aligned; never dereferenced on a rejected plan
    two = (_capi.tp_hd_image * 2)(_capi.tp_hd_image(0, 2, 2, 0, 0), _capi.tp_hd_image(4, 1, 1, 0, 725))   # 2x2 uses 5 crops
    assert lib.tp_hd_assemble(two, 2, fake, 6, None, fake, fake, fake, 2000, 144, 256, _capi.TP_BF16, None) == E
    assert "overlaps" in lib.tp_last_error().decode()
    two = (_capi.tp_hd_image * 2)(_capi.tp_hd_image(0, 2, 2, 0, 0), _capi.tp_hd_image(5, 1, 1, 0, 700))   # rows 0..724 taken
    assert lib.tp_hd_assemble(two, 2, fake, 6, None, fake, fake, fake, 2000, 144, 256, _capi.TP_BF16, None) == E
    two = (_capi.tp_hd_image * 2)(_capi.tp_hd_image(0, 2, 2, 0, 0), _capi.tp_hd_image(5, 1, 1, 0, 900))   # gap 725..899 is fine ...
    assert lib.tp_hd_assemble(two, 2, fake, 5, None, fake, fake, fake, 2000, 144, 256, _capi.TP_BF16, None) == E   # ... but crop 5 of 5 is not
    assert "crops up to 6 of 5" in lib.tp_last_error().decode()
    assert lib.tp_hd_assemble(two, 2, fake, 6, None, fake, fake, fake, 1000, 144, 256, _capi.TP_BF16, None) == E   # rows up to 1045 of 1000
    # status block of the packed weights, debug scan
    assert 0 < lib.tp_packed_status_offset(ctypes.byref(d)) < lib.tp_packed_weight_bytes(ctypes.byref(d))
    assert lib.tp_debug_count_saturated(ctypes.byref(d), None, 0, None, None) == E
    assert lib.tp_hd_slice(None, 100, 100, 1, 1, 336, 336, 0, 0, None, 336, None) == E
    # the test hooks live in libtokenpacker_exp.so (include/tokenpacker_test.h), not in the product library
    tl = _capi.load_test_library()
    assert tl.tp_test_occupy_cus(0, 1, None, None) == E
    assert tl.tp_test_pack_qr(None, None, None, None, None, None, None) == E          # (test hook of the pack-time QR)
    assert tl.tp_test_pack_qr_scratch_bytes() == 1024 * 1025 * 8 + 16 * 1024 * 8 + 16 * 8 + 256
    for sym in _capi.TEST_SYMBOLS:
        assert not hasattr(lib, sym), f"{sym} must not be exported by the product library"
    assert lib.tp_debug_counter(_capi.TP_COUNTER_SIDE_STREAMS) >= 0 and lib.tp_debug_counter(_capi.TP_COUNTER_PAIR_LAUNCHES) >= 0
    assert lib.tp_debug_counter(99) == -1
    # the timing-probe instantiations (garbage results) are not in the product library: its knob refuses them; the exp build takes them
    assert lib.tp_set_tuning(_capi.TP_TUNE_PAIR_DEBUG, 16) == E and "libtokenpacker_exp" in lib.tp_last_error().decode()
    assert lib.tp_set_tuning(_capi.TP_TUNE_PAIR_DEBUG, 0) == 0
    assert tl.tp_set_tuning(_capi.TP_TUNE_PAIR_DEBUG, 16) == 0 and tl.tp_set_tuning(_capi.TP_TUNE_PAIR_DEBUG, 0) == 0
    # the weight-gradient contraction on its own
    assert lib.tp_wgrad_workspace_bytes(1024, 4096) == 16 * 1024 * 4096 * 4
    assert lib.tp_wgrad_workspace_bytes(0, 4096) == 0
    assert lib.tp_wgrad(None, 1024, None, 4096, 0, 0, 4096, 1024, 4096, _capi.TP_BF16, None, _capi.TP_F32, 0, None, 0, None) == E


def test_tuning_keys_match_the_header():
    """Every TP_TUNE_* key of include/tokenpacker.h exists in the binding with the same number, the binding knows a default
    for each, and tp_set_tuning accepts exactly the keys below TP_TUNE_COUNT_."""
    src = open(os.path.join(ROOT, "include", "tokenpacker.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    keys = dict((k, int(v)) for k, v in re.findall(r"\b(TP_TUNE_[A-Z_0-9]+)\s*=\s*(\d+)", src))
    count = keys.pop("TP_TUNE_COUNT_")
    assert len(set(keys.values())) == len(keys) and max(keys.values()) < count
    for name, num in keys.items():
        assert getattr(_capi, name) == num, name
        assert num in _capi._TUNING_DEFAULTS, f"{name}: no default in _capi._TUNING_DEFAULTS"
    lib = _capi.load_library()
    assert lib.tp_set_tuning(count, 0) == _capi.TP_ERR_INVALID_ARG
    assert lib.tp_set_tuning(-1, 0) == _capi.TP_ERR_INVALID_ARG
    for num in keys.values():
        assert lib.tp_set_tuning(num, _capi._TUNING_DEFAULTS[num]) == _capi.TP_OK


def test_workspace_is_schedule_aware_and_an_upper_bound_for_the_tuning_at_call_time():
    """tp_workspace_bytes sizes the slabs the schedule of the moment writes (plan_schedule): the scale_factor-2 default has no
    H2 / K | V / Q1pre slab (1.2 GB less at B = 256); a masked forward (TP_DESC_MASKED), the unfused chain and the separate
    attention kernel need K | V or H2 again; the K-split partials exist only while TP_TUNE_SPLIT_K is not off."""
    lib = _capi.load_library()
    B, N, E = 256, 576, 1024
    slab = 2 * B * N * E * 2                       # one [2][B N, 1024] fp16 slab (H2, or K | V)

    def size(b=B, s=2, flags=0):
        d = _capi.make_desc(b, 24, s, 4096, _capi.TP_BF16, flags=flags)
        return lib.tp_workspace_bytes(ctypes.byref(d))
    base = size()
    a1 = B * 144 * E * 2                           # out_proj's output: the fold is off where K | V are rounded in front of attention
    try:
        assert slab <= size(flags=_capi.TP_DESC_MASKED) - base <= slab + a1 + 4096    # + K | V (+ A1)
        _capi.set_tuning(_capi.TP_TUNE_FUSE_ATTN, 1)
        assert slab <= size() - base <= slab + a1 + 4096                                 # separate attention kernel: + K | V (+ A1)
        _capi.set_tuning(_capi.TP_TUNE_FUSE_ATTN, 0)
        _capi.set_tuning(_capi.TP_TUNE_FUSE_KV_LN, 0)
        assert size() - base >= 2 * slab                                                 # + H2, + K | V, + Q1pre, (+ A1)
        _capi.set_tuning(_capi.TP_TUNE_FUSE_KV_LN, 1)
        assert size() == base
        # absorbed schedule (s = 3): u (one fp16 value per element) | qt (fp32) = 3 x [B M, 8, 1024] x 2 B instead of K | V, no H2, no logits
        assert size(s=3) < base + 3 * 8 * B * 64 * E * 2
        # K-split partials: only while the knob is on (the default), only for batches of at most 8 images
        partials = 512 * 128 * 128 * 4
        on = size(b=1)
        big_on = size(b=16)
        _capi.set_tuning(_capi.TP_TUNE_SPLIT_K, 2)
        assert partials <= on - size(b=1) < partials + 4096
        assert size(b=16) == big_on
        _capi.set_tuning(_capi.TP_TUNE_SPLIT_K, 0)
    finally:
        for k, v in _capi._TUNING_DEFAULTS.items():
            _capi.set_tuning(k, v)
    assert size(b=16) > size(b=9) and size() > 15 * size(b=16) // 2


def test_get_tuning_reads_the_library_table():
    lib = _capi.load_library()
    assert lib.tp_get_tuning(99) == -1 and lib.tp_get_tuning(-1) == -1
    for k, v in _capi._TUNING_DEFAULTS.items():
        assert _capi.get_tuning(k) == v, k
    try:
        assert lib.tp_set_tuning(_capi.TP_TUNE_RESERVE_CUS, 3) == _capi.TP_OK        # a direct call, past the wrapper
        assert _capi.get_tuning(_capi.TP_TUNE_RESERVE_CUS) == 3
    finally:
        _capi.set_tuning(_capi.TP_TUNE_RESERVE_CUS, 0)


def test_gather_entry_points_reject_bad_arguments():
    lib = _capi.load_library()
    E = _capi.TP_ERR_INVALID_ARG
    off = ctypes.c_uint64(0)
    assert lib.tp_gather_export(None, None, ctypes.byref(off)) == E
    assert lib.tp_gather_open(None, None) == E
    assert lib.tp_gather_close(None) == E
    assert lib.tp_gather_alloc_flags(None, 256) == E and lib.tp_gather_free_flags(None) == E
    assert lib.tp_gather_sync(None, 2, 0, 0, None, 0, None, 0, None) == E
    fake = ctypes.c_void_p(4096)
    assert lib.tp_gather_sync(fake, 0, 0, 0, None, 0, None, 0, None) == E          # world < 1
    assert lib.tp_gather_sync(fake, 65, 0, 0, None, 0, None, 0, None) == E         # one wave polls at most 64 sources
    assert lib.tp_gather_sync(fake, 2, 2, 0, None, 0, None, 0, None) == E          # rank out of range
    assert lib.tp_gather_push(1, None, fake, 16, None, fake, None, 0) == E
    assert lib.tp_gather_push(0, None, None, 0, None, None, None, 0) == E          # no sequence cell
    assert _capi.TP_IPC_HANDLE_BYTES == 64


def test_tuning_contexts_are_private_copies():
    """ABI 4: tp_tuning_create copies the process-wide table of the moment; setting a context does not touch the table or another
    context; an entry point that takes a tp_desc reads desc->tuning (here: the workspace size follows the context's SPLIT_K, not the
    table's); bad keys / NULL are errors."""
    lib = _capi.load_library()
    a, b = _capi.TuningContext(), _capi.TuningContext(split_k=2)
    try:
        for k, v in _capi._TUNING_DEFAULTS.items():
            assert a.get(k) == v
        assert b.get(_capi.TP_TUNE_SPLIT_K) == 2 and a.get(_capi.TP_TUNE_SPLIT_K) == 0 and _capi.get_tuning(_capi.TP_TUNE_SPLIT_K) == 0
        size = lambda t: lib.tp_workspace_bytes(ctypes.byref(_capi.make_desc(1, 24, 2, 4096, _capi.TP_BF16, tuning=t)))
        partials = 512 * 128 * 128 * 4
        assert size(None) == size(a) and partials <= size(a) - size(b) < partials + 4096
        _capi.set_tuning(_capi.TP_TUNE_SPLIT_K, 2)                  # the table changes under the contexts' feet: they do not move
        try:
            assert size(None) == size(b) and size(a) - size(b) >= partials and a.get(_capi.TP_TUNE_SPLIT_K) == 0
            c = _capi.TuningContext()                               # ... and a NEW context starts from the table of the moment
            assert c.get(_capi.TP_TUNE_SPLIT_K) == 2
            c.close()
        finally:
            _capi.set_tuning(_capi.TP_TUNE_SPLIT_K, 0)
        assert lib.tp_tuning_set(a.handle, _capi.TP_TUNE_COUNT, 0) == _capi.TP_ERR_INVALID_ARG
        assert lib.tp_tuning_set(None, 0, 0) == _capi.TP_ERR_INVALID_ARG and lib.tp_tuning_get(None, 0) == -1
    finally:
        a.close(); b.close()
    # a CLOSED context must not silently fall back to the process-wide table: the caller asked for ITS knobs
    import pytest
    with pytest.raises(ValueError, match="closed"):
        _capi.make_desc(1, 24, 2, 4096, _capi.TP_BF16, tuning=a)
    assert _capi.make_desc(1, 24, 2, 4096, _capi.TP_BF16, tuning=None).tuning is None      # (None stays "the table")


def test_gemm_routing_policy_is_host_logic_and_pinned():
    """Where tp_linear sends a launch is decided on the host by counting CU rounds (tp_gemm.hip: gemm_route / gemm_takes_pair_route);
    tp_test_gemm_route exposes the decision (256 CUs are assumed without a device).  The B = 256 forward runs full 256 x 256 tiles
    (its query-side GEMMs the pair kernel); a 32-image shard's first layer and mlp launches take the 192 x 256 tiles that make them
    whole rounds; one image runs on the 128-tile kernel; statistics-only launches never take the 192-row tiles (not built for them)."""
    lib = _capi.load_test_library()                      # (tp_test_gemm_route: include/tokenpacker_test.h; the exp library's OWN tuning table)
    set_tuning = lambda k, v: lib.tp_set_tuning(k, v)     # noqa: E731
    G, S, NS = _capi.TP_LINEAR_GELU, _capi.TP_LINEAR_ROW_STATS, _capi.TP_LINEAR_NO_STORE
    SMALL, FULL, HALF, SPLIT, T192, PAIR = range(6)
    r = lambda M, N, K, flags=0, groups=1: lib.tp_test_gemm_route(M, N, K, flags, groups)  # noqa: E731
    assert r(0, 256, 256) == -1 and r(256, 100, 256) == -1
    # B = 256 (147456 key rows, 36864 query rows)
    assert r(147456, 2048, 4096, G) == FULL and r(36864, 4096, 4096) == FULL and r(36864, 4096, 1024, G) == FULL
    assert r(147456, 1024, 1024, S | NS, 2) == FULL
    assert r(36864, 1024, 1024) == PAIR
    # the 8-GPU shard: 32 images
    assert r(18432, 2048, 4096, G) == T192 and r(4608, 4096, 4096) == T192 and r(4608, 4096, 1024, G) == T192
    assert r(18432, 1024, 1024, S | NS, 2) != T192
    # one image
    assert r(576, 2048, 4096, G) == SMALL and r(144, 4096, 4096) == SMALL
    # the A/B switches
    set_tuning(_capi.TP_TUNE_GEMM_TILE, 4)
    try:
        assert r(18432, 2048, 4096, G) == SPLIT and r(4608, 4096, 4096) in (SPLIT, HALF)
    finally:
        set_tuning(_capi.TP_TUNE_GEMM_TILE, 0)
    set_tuning(_capi.TP_TUNE_PAIR_GEMM, 1)
    try:
        assert r(36864, 1024, 1024) != PAIR
    finally:
        set_tuning(_capi.TP_TUNE_PAIR_GEMM, 0)
    set_tuning(_capi.TP_TUNE_GEMM_TILE, 3)
    try:
        assert r(147456, 2048, 4096, G) == T192 and r(147456, 1024, 1024, S | NS, 2) != T192
    finally:
        set_tuning(_capi.TP_TUNE_GEMM_TILE, 0)


def test_tp_linear_refuses_the_training_flags():
    """TP_LINEAR_SAVE_PRE / TP_LINEAR_GELU_BWD need a pre-activation buffer tp_linear_args has no field for: tp_linear refuses
    them on the host (a launch would address that buffer from NULL).  The message is asserted as well as the status."""
    lib = _capi.load_library()
    fake = 4096                                                      # non-NULL, 16-byte aligned; never dereferenced on a refusal
    for flag, name in ((_capi.TP_LINEAR_SAVE_PRE, "TP_LINEAR_SAVE_PRE"), (_capi.TP_LINEAR_GELU_BWD, "TP_LINEAR_GELU_BWD")):
        for extra in (0, _capi.TP_LINEAR_GELU):
            a = _capi.tp_linear_args()
            a.M, a.N, a.K, a.dtype, a.out_dtype = 256, 256, 64, _capi.TP_F16, _capi.TP_F16
            a.lda, a.ldc, a.A, a.W, a.C, a.bias = 64, 256, fake, fake, fake, fake
            a.flags = flag | extra
            assert lib.tp_linear(ctypes.byref(a), None) == _capi.TP_ERR_INVALID_ARG
            msg = lib.tp_last_error().decode()
            assert name in msg and "training entry points" in msg, msg


def test_backward_kernel_hooks_refuse_bad_arguments():
    """Every tp_test_bw_* / tp_test_region_attention* / tp_test_point_queries_bwd / tp_test_linear_bwd hook turns a mistaken call — NULL, misaligned, a count
    that is not a multiple of 8 / 4, a scratch too small — into TP_ERR_INVALID_ARG on the host (include/tokenpacker_test.h)."""
    tl = _capi.load_test_library()
    E = _capi.TP_ERR_INVALID_ARG
    F16, BF16, F32 = _capi.TP_F16, _capi.TP_BF16, _capi.TP_F32
    p, odd = 4096, 4104                                               # fake device pointers: aligned | 8 bytes off; never dereferenced
    big = 1 << 30

    def refused(fn, good, bad_variants):
        for i, val in bad_variants:
            args = list(good)
            args[i] = val
            assert fn(*args) == E, (fn.__name__, i, val)
            msg = tl.tp_last_error().decode()                         # (the hook's own refusal, or its launcher's host-side one)
            assert msg.startswith((fn.__name__, "bw ", "tp gemm")), msg

    # (src_dtype, dst_dtype, src, ld, rows_per_batch, batch_stride, R, C, dst, ldd, Rpad, mean_rstd, gamma, beta, colsum_part, colsum_floats, stream)
    refused(tl.tp_test_bw_transpose, [F16, BF16, p, 64, 0, 0, 100, 64, p, 104, 104, None, None, None, None, 0, None],
            [(2, None), (8, None), (2, odd), (8, odd), (0, F32), (1, 7), (3, 60), (3, 56), (7, 60), (9, 100), (10, 100), (10, 96), (6, 0),
             (11, p), (14, p), (4, 50)])
    refused(tl.tp_test_bw_transpose, [F16, F16, p, 64, 50, 3200, 100, 64, p, 104, 104, None, None, None, p, 2 * 64, None],
            [(5, 3196), (5, 1600), (15, 2 * 64 - 1)])
    arr = lambda t, v: (t * len(v))(*v)                               # noqa: E731
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    good = [F16, F16, 2, arr(vp, [p, p]), arr(i64, [64, 64]), arr(i32, [10, 10]), arr(i32, [64, 64]), arr(vp, [p, p]), arr(i32, [16, 16]), None]
    refused(tl.tp_test_bw_transpose_batch, good,
            [(2, 0), (2, 9), (0, F32), (3, None), (7, None), (3, arr(vp, [p, None])), (3, arr(vp, [p, odd])), (8, arr(i32, [16, 8])),
             (8, arr(i32, [16, 12])), (4, arr(i64, [64, 60])), (6, arr(i32, [64, 60]))])
    cnt = ctypes.c_int(0)
    # (dtype, src, ld, R, C, part, part_floats, amax_part, amax_floats, amax_count, stream)
    refused(tl.tp_test_bw_colsum_rows, [BF16, p, 1024, 4096, 1024, p, 64 * 1024, p, 4096, ctypes.byref(cnt), None],
            [(1, None), (5, None), (1, odd), (0, F32), (2, 1020), (2, 512), (4, 1020), (3, 0), (6, 64 * 1024 - 1), (8, 4095), (9, None)])
    # (dst_dtype, part, part_stride, nparts, n, out, out_scale, stream)
    refused(tl.tp_test_bw_reduce_parts, [F32, p, 1024, 4, 1024, p, None, None],
            [(1, None), (5, None), (1, odd), (5, odd), (0, 9), (3, 0), (4, 0), (2, 1000)])
    # (dst_dtype, part, part_stride, nparts, n, out, scratch, scratch_floats, out_scale, n_out, stream)
    refused(tl.tp_test_bw_reduce_many_parts, [BF16, p, 1024, 300, 1024, p, p, 32 * 1024, None, -1, None],
            [(1, None), (5, None), (6, None), (1, odd), (6, odd), (0, 5), (3, 0), (4, 1022), (2, 1022), (2, 1020), (7, 32 * 1024 - 1), (9, 1025),
             (9, -2)])
    refused(tl.tp_test_bw_dynamic_scale, [p, 8, p, None], [(0, None), (2, None), (1, 0)])
    # (src_dtype, src, n, scale, dst_f16, sat_flag, stream)
    refused(tl.tp_test_bw_scale_cast, [BF16, p, 1024, p, p, None, None], [(1, None), (3, None), (4, None), (0, F32), (2, 0)])
    for i, val in ((2, 1020), (1, odd), (4, odd)):                    # (the launcher's own checks)
        args = [BF16, p, 1024, p, p, None, None]
        args[i] = val
        assert tl.tp_test_bw_scale_cast(*args) == E
    # (gdtype, dy, x, mean_rstd, gamma, dx, part, part_floats, nblocks, rows, beta, xn, sat_flag, stream)
    refused(tl.tp_test_bw_ln_backward, [F16, p, p, p, p, p, p, 7 * 3072, 7, 100, None, None, None, None],
            [(1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (1, odd), (2, odd), (5, odd), (0, F32), (7, 7 * 3072 - 1),
             (8, 0), (8, 70000), (9, 0), (11, odd)])
    args = [F16, p, p, p, p, p, p, 7 * 3072, 7, 100, None, p, None, None]     # xn without beta: the launcher's check
    assert tl.tp_test_bw_ln_backward(*args) == E
    # (gdtype, q, k, v, dout, dq, dk, dv, B, grid, s, mask, mask_mode, dmask, inv_scale, part, part_bytes, redscratch, redscratch_floats, sat_flag, stream)
    good = [BF16, p, p, p, p, p, p, p, 2, 24, 3, None, 0, None, None, None, 0, None, 0, None, None]
    refused(tl.tp_test_bw_region_attention, good,
            [(i, None) for i in range(1, 8)] + [(i, odd) for i in range(1, 8)] + [(0, F32), (8, 0), (10, 5), (10, 0), (12, 3), (11, p), (13, p),
                                                                                 (12, 1), (12, 2)])
    good = [BF16, p, p, p, p, p, p, p, 2, 24, 3, p, 1, p, None, p, 2 * 64 * 12 * 4, p, 32 * 12, None, None]
    refused(tl.tp_test_bw_region_attention, good, [(15, None), (17, None), (15, odd), (13, odd), (16, 2 * 64 * 12 * 4 - 1), (18, 32 * 12 - 1)])
    # (q, k, v, o, B, grid, s, mask, mask_mode, region_major, stream)
    refused(tl.tp_test_region_attention, [p, p, p, p, 2, 24, 3, None, 0, 0, None],
            [(i, None) for i in range(4)] + [(i, odd) for i in range(4)] + [(4, 0), (5, 0), (6, 5), (6, 0), (5, 2048), (7, p), (8, 1), (8, 2), (8, 3),
                                                                           (8, -1), (9, 2), (9, -1)])
    refused(tl.tp_test_region_attention, [p, p, p, p, 2, 24, 3, p, 2, 1, None], [(7, None), (7, p + 2), (8, 0)])
    # (qt, h2k, h2v, mr_k, mr_v, u, B, grid, s, mask, mask_mode, stream)
    refused(tl.tp_test_region_attention_absorbed, [p, p, p, p, p, p, 2, 24, 3, None, 0, None],
            [(i, None) for i in range(6)] + [(i, odd) for i in (0, 1, 2, 5)] + [(3, p + 4), (4, p + 4), (6, 0), (8, 5), (8, 0), (9, p), (10, 1), (10, 3)])
    assert tl.tp_test_region_attention_absorbed(p, p, p, p, p, p, 1, 18, 9, None, 0, None) == E       # (the launcher's refusal: 81 keys)
    assert "keys > 64" in tl.tp_last_error().decode()
    # (dtype, dq0, inv_scale, dx, B, grid, s, stream)
    refused(tl.tp_test_point_queries_bwd, [F16, p, None, p, 1, 24, 2, None], [(1, None), (3, None), (1, odd), (3, odd), (0, F32), (4, 0), (6, 5), (6, 0)])
    # (M, N, K, dtype, out_dtype, flags, A, lda, W, C, ldc, Z, ldz, out_scale, tile, stream)
    good = [256, 256, 64, F16, F16, _capi.TP_LINEAR_GELU_BWD, p, 64, p, p, 256, p, 512, None, 128, None]
    refused(tl.tp_test_linear_bwd, good,
            [(6, None), (8, None), (9, None), (11, None), (6, odd), (9, odd), (11, odd), (3, F32), (4, 9), (5, _capi.TP_LINEAR_GELU), (5, 16),
             (7, 60), (7, 56), (10, 250), (10, 128), (12, 250), (12, 128), (14, 64), (0, 0)])
    assert tl.tp_test_linear_bwd(256, 256, 64, F16, F16, 0, p, 64, p, p, 256, p, 256, None, 0, None) == E        # Z without the flag
    assert tl.tp_test_linear_bwd(256, 200, 64, F16, F16, 0, p, 64, p, p, 256, None, 0, None, 0, None) == E       # (gemm_launch: N % 128)
    # the training epilogue exists for 16-bit outputs only: refused on the host by the GEMM launchers, on either tile
    for tile in (128, 256):
        assert tl.tp_test_linear_bwd(256, 256, 128, F16, F32, _capi.TP_LINEAR_GELU_BWD, p, 128, p, p, 256, p, 256, None, tile, None) == E
        assert "16-bit output" in tl.tp_last_error().decode()
        assert tl.tp_test_linear_bwd(256, 256, 128, F16, F32, 0, p, 128, p, p, 256, None, 0, p, tile, None) == E


def _packed_layout_fields():
    """The fields of PackedLayout, in declaration order, from csrc/tp_internal.h itself."""
    src = open(os.path.join(ROOT, "tokenpacker_amd", "csrc", "tp_internal.h")).read()
    body = re.search(r"struct PackedLayout \{(.*?)\n\};", src, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return [n.strip() for decl in re.findall(r"size_t ([^;]+);", body) for n in decl.split(",")]


@pytest.mark.parametrize("hidden", [384, 4096])
def test_packed_layout_hook(hidden):
    """tp_test_packed_layout (include/tokenpacker_test.h, host logic only): every PackedLayout field resolves; offsets are 256-byte
    aligned and strictly increasing in declaration order; the reserved ranges do not overlap; `status` and `total` are what the
    product ABI reports; a bad name or width is refused."""
    from tests import pack_ref
    lib, tl = _capi.load_library(), _capi.load_test_library()
    fields = _packed_layout_fields()
    assert fields[0] == "w_kv0" and fields[-2:] == ["status", "total"] and len(fields) == len(set(fields)) == 38
    assert fields[:-1] == list(pack_ref.field_specs(hidden))                 # the tests' own table names the same fields in the same order
    d = _capi.make_desc(1, 24, 2, hidden, _capi.TP_BF16)
    off, nbytes = ctypes.c_size_t(), ctypes.c_size_t()
    lay = []
    for name in fields:
        assert tl.tp_test_packed_layout(hidden, name.encode(), ctypes.byref(off), ctypes.byref(nbytes)) == _capi.TP_OK, name
        lay.append((name, off.value, nbytes.value))
    assert lay[0][1] == 0
    for (name, o, n), (_, nxt, _) in zip(lay[:-1], lay[1:]):
        assert o % 256 == 0 and n > 0, name
        assert o < nxt and o + n <= nxt, f"{name} [{o}, {o + n}) runs into the next field at {nxt}"
        assert nxt - (o + n) < 256, name                                     # (nothing but alignment padding in between)
    by_name = {name: (o, n) for name, o, n in lay}
    assert by_name["status"] == (lib.tp_packed_status_offset(ctypes.byref(d)), 256)
    assert by_name["total"] == (lib.tp_packed_weight_bytes(ctypes.byref(d)), 0)
    assert by_name["w_m2"][1] == hidden * hidden * 2 and by_name["w_cc_v3"][1] == 2 * 1024 * 1024 * 2
    E = _capi.TP_ERR_INVALID_ARG
    assert tl.tp_test_packed_layout(hidden, b"w_kv1", ctypes.byref(off), ctypes.byref(nbytes)) == E
    assert "w_kv1" in tl.tp_last_error().decode()
    assert tl.tp_test_packed_layout(hidden + 64, b"w_kv0", ctypes.byref(off), ctypes.byref(nbytes)) == E
    assert "multiple of 128" in tl.tp_last_error().decode()
    assert tl.tp_test_packed_layout(0, b"w_kv0", ctypes.byref(off), ctypes.byref(nbytes)) == E
    assert tl.tp_test_packed_layout(hidden, None, ctypes.byref(off), ctypes.byref(nbytes)) == E
