"""The backward into a gradient sink on a real MI355X (tp_backward_sink; ``TokenPacker``'s frozen parameters and ``use_main_grad``):
the full model-dtype sink IS tp_backward, a partial sink gives every wanted gradient the full backward's bits and computes nothing
for the rest, an fp32 sink holds the sum the model-dtype gradient is rounded from, an accumulating sink is torch's ``c + g`` bit for
bit, and ``main_grad`` accumulation over micro-batches stays within the parameter gradients' gate against fp64 autograd."""
import ctypes

import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tokenpacker_amd import TokenPacker, _capi, synth

pytestmark = pytest.mark.gpu

GATE_L2 = 1e-2                     # the parameter gradients' gate (test_gpu_backward.py)
NAMES = _capi.WEIGHT_FIELDS
_TP = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16, torch.float32: _capi.TP_F32}

MLP2 = ("mlp.2.weight", "mlp.2.bias")
MLP = MLP2 + ("mlp.0.weight", "mlp.0.bias")
K_BRANCH = tuple(n for n in NAMES if n.startswith(("k_proj_1.", "ln_k_1.")))
KV = tuple(n for n in NAMES if n.startswith(("k_proj_1.", "v_proj_1.", "ln_k_1.", "ln_v_1.")))
NOT_KV = tuple(n for n in NAMES if n not in KV)


def _module(params, D, s, dtype, grid=24):
    m = TokenPacker(raw_grid=grid, hidden_size=D, scale_factor=s)
    m.load_state_dict(params)
    return m.to(device="cuda", dtype=dtype).train()


def _inputs(seed, B, dtype, grid, s, D):
    """-> (x, x_multi, w) on the CPU in ``dtype``; synth's features for the 24 x 24 grid, as in test_gpu_backward.py."""
    g = torch.Generator().manual_seed(seed + 2)
    if grid == 24:
        x, xm = synth.make_inputs(seed + 1, B, dtype)
    else:
        x = torch.randn(B, grid * grid, 1024, generator=g).to(dtype)
        xm = torch.randn(B, grid * grid, 4096, generator=g).to(dtype)
    w = torch.randn(B, (grid // s) ** 2, D, generator=g).to(dtype)
    return x, xm, w


def _errors(got, want):
    """test_gpu_backward.py's metric: rms error over max(rms(g_ref), 0.1 * the largest rms among same-shaped parameters) — some
    gradients (ln_k_1.bias, the k third of in_proj_bias) are mathematically zero."""
    rms = {k: float(v.norm()) / v.numel() ** 0.5 for k, v in want.items()}
    out = {}
    for k in want:
        scale = max(rms[k], 0.1 * max(rms[j] for j in want if want[j].shape == want[k].shape))
        out[k] = float((got[k].double().cpu() - want[k]).norm()) / want[k].numel() ** 0.5 / scale
    return out


def _oracle_grads(params, x, xm, w, s, dtype, grid=24):
    """fp64 autograd on the same rounded weights and inputs (CPU): d sum(y * w) / d parameter."""
    ref_p = {k: v.to(dtype).double().requires_grad_(True) for k, v in params.items()}
    y = orc.forward(ref_p, x, xm, scale_factor=s, raw_grid=grid, compute_dtype=torch.float64, io_dtype=dtype)
    (y * w.double()).sum().backward()
    return {k: v.grad for k, v in ref_p.items()}


class _Step:
    """One training forward on the device, kept for any number of direct C-ABI backward calls on it (the training workspace is
    read-only for the backward).  The backward workspace is filled with finite garbage before every call: a stage that was skipped
    leaves it there, and nothing wanted may depend on it."""

    def __init__(self, m, x, xm, dy, mask=None):
        self.m, self.lib = m, _capi.load_library()
        self.x, self.xm, self.dy = x.cuda().contiguous(), xm.cuda().contiguous(), dy.cuda().contiguous()
        self.mask = mask
        self.out, self.ws, self.desc, self.packed = m._launch_forward(self.x, self.xm, train=True, mask=mask)
        self.params = [p.detach().contiguous() for p in m._named_weights()]
        self.raw = _capi.tp_weights(*[t.data_ptr() for t in self.params])
        nbytes = self.lib.tp_backward_inputs_workspace_bytes(ctypes.byref(self.desc))
        assert nbytes >= self.lib.tp_backward_workspace_bytes(ctypes.byref(self.desc)) > 0
        self.bw = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.strides = _capi.strides3(self.xm.stride())
        self.stream = torch.cuda.current_stream().cuda_stream

    def buffers(self, dtype=None, names=NAMES, fill=None):
        """One gradient buffer per named parameter (None for the others)."""
        out = []
        for n, p in zip(NAMES, self.params):
            t = None
            if n in names:
                t = torch.empty(p.shape, dtype=dtype or p.dtype, device="cuda")
                t.fill_(float("nan")) if fill is None else t.copy_(fill[n])
            out.append(t)
        return out

    def _common(self):
        self.bw.fill_(0x3C)
        return (ctypes.byref(self.raw), self.packed.data_ptr(), self.ws.data_ptr(), self.dy.data_ptr())

    @staticmethod
    def _grads(bufs):
        return _capi.tp_grads(*[None if t is None else t.data_ptr() for t in bufs])

    def legacy(self, bufs=None, ig=None, am=None):
        """tp_backward / tp_backward_inputs / tp_backward_masked, whichever the arguments call for."""
        g = ctypes.byref(self._grads(bufs)) if bufs is not None else None
        d, xm, st = ctypes.byref(self.desc), self.xm.data_ptr(), self.strides
        tail = (self.bw.data_ptr(), self.bw.numel(), self.stream)
        if am is not None:
            rc, what = self.lib.tp_backward_masked(d, xm, None, st, *self._common(), g, None if ig is None else ctypes.byref(ig),
                                                   ctypes.byref(am), *tail), "tp_backward_masked"
        elif ig is not None:
            rc, what = self.lib.tp_backward_inputs(d, xm, st, *self._common(), g, ctypes.byref(ig), *tail), "tp_backward_inputs"
        else:
            rc, what = self.lib.tp_backward(d, xm, st, *self._common(), g, *tail), "tp_backward"
        _capi.check(rc, what)

    def sink(self, bufs, dtype=None, accumulate=0, ig=None, am=None):
        """tp_backward_sink with one entry per non-None buffer (``bufs`` None: an all-NULL sink)."""
        bufs = bufs if bufs is not None else [None] * len(NAMES)
        sk = _capi.tp_grad_sink(self._grads(bufs), _TP[dtype] if dtype is not None else self.desc.dtype, accumulate)
        _capi.check(self.lib.tp_backward_sink(ctypes.byref(self.desc), self.xm.data_ptr(), None, self.strides, *self._common(),
                                              ctypes.byref(sk), None if ig is None else ctypes.byref(ig),
                                              None if am is None else ctypes.byref(am), self.bw.data_ptr(), self.bw.numel(),
                                              self.stream), "tp_backward_sink")


def _step(dtype, s, D, B, seed, grid=24, mask=None):
    params = synth.make_params(seed, D)
    x, xm, w = _inputs(seed, B, dtype, grid, s, D)
    return _Step(_module(params, D, s, dtype, grid), x, xm, w, mask=mask), (params, x, xm, w)


# ---- 1. the full sink is tp_backward ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,s,D,B,grid", [
    (torch.bfloat16, 2, 256, 2, 24), (torch.float16, 2, 256, 2, 24), (torch.bfloat16, 3, 256, 3, 24),
    (torch.bfloat16, 2, 384, 2, 24),      # D not a multiple of 256: the transposed-operand fallback of the mlp weight gradients
    (torch.bfloat16, 2, 256, 7, 8)])      # 64 tokens per image: the first layer's transposed-copy path
def test_full_sink_equals_tp_backward(dtype, s, D, B, grid):
    st, _ = _step(dtype, s, D, B, 50 + s + grid, grid)
    a, b = st.buffers(), st.buffers()
    st.legacy(a)
    st.sink(b)
    torch.cuda.synchronize()
    for n, ga, gb in zip(NAMES, a, b):
        assert torch.isfinite(ga).all(), n
        assert torch.equal(ga, gb), n
    assert int(st.bw[:4].view(torch.int32).item()) == 0          # (the status word keeps its meaning: nothing saturated)


# ---- 2. frozen subsets through the module -----------------------------------------------------------------------------------
def _train_once(params, x, xm, w, D, s, dtype, trainable, spy=None):
    """-> {name: .grad or None} of one step of a module whose parameters outside ``trainable`` are frozen."""
    m = _module(params, D, s, dtype)
    for n, p in m.named_parameters():
        p.requires_grad_(n in trainable)
    if spy is not None:
        lib = _capi.load_library()
        real = lib.tp_backward_sink

        def recording(*args):
            spy.append(args[8]._obj)                              # the tp_grad_sink behind byref()
            return real(*args)
        lib.tp_backward_sink = recording
    try:
        (m((x.cuda(), xm.cuda())).float() * w.cuda().float()).sum().backward()
        torch.cuda.synchronize()
    finally:
        if spy is not None:
            lib.tp_backward_sink = real
    return {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}


_FULL = {}


def _full_run(dtype, s, D, B):
    """The all-trainable step of a shape, computed once and shared by every subset of it."""
    key = (dtype, s, D, B)
    if key not in _FULL:
        params = synth.make_params(60 + s, D)
        x, xm, w = _inputs(60 + s, B, dtype, 24, s, D)
        _FULL[key] = ((params, x, xm, w), _train_once(params, x, xm, w, D, s, dtype, NAMES))
    return _FULL[key]


SUBSETS = {"all": NAMES, "mlp2": MLP2, "mlp": MLP, "q_proj": ("q_proj_1.weight",), "k_branch": K_BRANCH,
           "in_proj_weight": ("clip_attn.in_proj_weight",), "v0_bias": ("v_proj_1.0.bias",), "not_kv": NOT_KV}


@pytest.mark.parametrize("s,D,B,subset", [(2, 256, 2, k) for k in SUBSETS] + [(4, 512, 2, "not_kv")])
def test_frozen_subsets_through_the_module(s, D, B, subset):
    dtype, trainable = torch.bfloat16, SUBSETS[subset]
    (params, x, xm, w), full = _full_run(dtype, s, D, B)
    sinks = []
    got = _train_once(params, x, xm, w, D, s, dtype, trainable, spy=sinks)
    assert len(sinks) == 1 and sinks[0].dtype == _capi.TP_BF16 and sinks[0].accumulate == 0
    for n in NAMES:
        entry = getattr(sinks[0].grads, n.replace(".", "_"))
        if n in trainable:
            assert entry, n                                       # a buffer was handed over ...
            assert torch.equal(got[n], full[n]), n                # ... and holds the all-trainable run's bits
        else:
            assert entry is None, n                               # NULL: neither computed nor allocated
            assert got[n] is None, n
    plan = set(_capi.backward_plan(trainable))                    # what the library ran for this sink
    if subset == "not_kv":
        assert not plan & {"DZ1", "KV0_WGRAD"}
    if subset in ("mlp2", "mlp"):
        assert not plan & {"DA1", "DO", "ATTENTION", "Q_CHAIN", "K_CHAIN", "V_CHAIN", "DZ1", "KV0_WGRAD"}


# ---- 3. the fp32 sink, overwrite ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bf16_step():
    """(2, 256, 2) in bf16: the step, its model-dtype gradients g (tp_backward) and its fp32 gradients g32 (fp32 sink, overwrite)."""
    st, case = _step(torch.bfloat16, 2, 256, 2, 70)
    g, g32 = st.buffers(), st.buffers(torch.float32)
    st.legacy(g)
    st.sink(g32, torch.float32)
    torch.cuda.synchronize()
    return st, case, dict(zip(NAMES, g)), dict(zip(NAMES, g32))


def test_fp32_sink_rounds_to_the_model_dtype_gradient_bf16(bf16_step):
    st, (params, x, xm, w), g, g32 = bf16_step
    for n in NAMES:
        assert g32[n].dtype == torch.float32 and torch.isfinite(g32[n]).all(), n
        assert torch.equal(g32[n].to(torch.bfloat16), g[n]), n    # one fp32 sum; the model-dtype path rounds it once
    errs = _errors(g32, _oracle_grads(params, x, xm, w, 2, torch.bfloat16))
    for n, e in errs.items():
        print(f"[sink fp32] bf16 {n:30s} rel_l2={e:.3e}")
        assert e <= GATE_L2, (n, e)


def test_fp32_sink_rounds_to_the_model_dtype_gradient_fp16():
    st, (params, x, xm, w) = _step(torch.float16, 2, 256, 2, 71)
    g, g32 = st.buffers(), st.buffers(torch.float32)
    st.legacy(g)
    st.sink(g32, torch.float32)
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, g, g32):
        assert torch.equal(b.to(torch.float16), a), n
    errs = _errors(dict(zip(NAMES, g32)), _oracle_grads(params, x, xm, w, 2, torch.float16))
    for n, e in errs.items():
        print(f"[sink fp32] fp16 {n:30s} rel_l2={e:.3e}")
        assert e <= GATE_L2, (n, e)


# ---- 4. accumulate ----------------------------------------------------------------------------------------------------------
def _pattern(st):
    """A known fp32 pattern per parameter, of the gradients' own magnitude and with every mantissa bit in use."""
    g = torch.Generator().manual_seed(4)
    return {n: torch.randn(p.shape, generator=g).cuda() * 0.37 for n, p in zip(NAMES, st.params)}


def _accumulate_twice(st1, st2, c, names=NAMES):
    acc = st1.buffers(torch.float32, names=names, fill=c)
    st1.sink(acc, torch.float32, accumulate=1)
    # (the second step's buffers are the first's: same addresses, another step's forward, inputs and dy)
    st2.sink(acc, torch.float32, accumulate=1)
    torch.cuda.synchronize()
    return dict(zip(NAMES, acc))


def test_accumulate_is_torch_addition_bit_for_bit(bf16_step):
    st1, _, _, g1 = bf16_step
    x, xm, w = _inputs(170, 2, torch.bfloat16, 24, 2, 256)        # other inputs, another dy (and another dynamic scale: 8 x larger)
    st2 = _Step(st1.m, x, xm, w * 8)
    g2 = dict(zip(NAMES, st2.buffers(torch.float32)))
    st2.sink(list(g2.values()), torch.float32)
    c = _pattern(st1)
    acc = _accumulate_twice(st1, st2, c)
    for n in NAMES:
        assert not torch.equal(g1[n], g2[n]), n
        assert torch.equal(acc[n], (c[n] + g1[n]) + g2[n]), n
    # 7. determinism: the same sequence again gives the same bits
    again = _accumulate_twice(st1, st2, c)
    assert all(torch.equal(acc[n], again[n]) for n in NAMES)
    # a partial accumulating sink: the wanted entries as above, and nothing else is touched (there is nothing else to touch)
    part = _accumulate_twice(st1, st2, c, names=K_BRANCH)
    for n in NAMES:
        assert (part[n] is None) if n not in K_BRANCH else torch.equal(part[n], acc[n]), n


# ---- 5. use_main_grad ---------------------------------------------------------------------------------------------------------
def test_use_main_grad_accumulates_micro_batches_in_fp32():
    dtype, s, D, B, n_micro = torch.bfloat16, 2, 256, 2, 3
    params = synth.make_params(80, D)
    micro = [_inputs(80 + 10 * i, B, dtype, 24, s, D) for i in range(n_micro)]
    m_main, m_plain = _module(params, D, s, dtype), _module(params, D, s, dtype)
    m_main.use_main_grad = True
    with pytest.raises(TypeError, match="has no main_grad"):      # (named, before anything is launched)
        m_main((micro[0][0].cuda(), micro[0][1].cuda()))
    m_main.init_main_grads()
    for x, xm, w in micro:                                        # (no zeroing in between: every call accumulates)
        for m in (m_main, m_plain):
            (m((x.cuda(), xm.cuda())).float() * w.cuda().float()).sum().backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m_main.parameters())       # the Megatron convention: autograd is told nothing
    x, xm, w = (torch.cat(t) for t in zip(*micro))                # (no operation mixes images: one fp64 run gives the summed gradient)
    want = _oracle_grads(params, x, xm, w, s, dtype)
    e_main = _errors({n: p.main_grad for n, p in m_main.named_parameters()}, want)
    e_plain = _errors({n: p.grad for n, p in m_plain.named_parameters()}, want)
    for n in NAMES:
        print(f"[main_grad] {n:30s} rel_l2: fp32 main_grad {e_main[n]:.3e} | bf16 .grad += {e_plain[n]:.3e}")
    print(f"[main_grad] worst: fp32 main_grad {max(e_main.values()):.3e} | bf16 .grad += {max(e_plain.values()):.3e}")
    for n in NAMES:
        assert m_main.get_parameter(n).main_grad.dtype == torch.float32
        assert e_main[n] <= GATE_L2, (n, e_main[n])
    m_main.zero_main_grads()
    assert all(float(p.main_grad.abs().max()) == 0.0 for p in m_main.parameters())


# ---- 6. a masked case and an inputs case through the sink -----------------------------------------------------------------------
def test_mask_gradient_alone_equals_tp_backward_masked():
    """The projector frozen, only dL/dmask wanted (the chain stops after the attention backward)."""
    mask = (0.5 * torch.randn(4, generator=torch.Generator().manual_seed(6))).cuda()       # mode 1: [s * s]
    st, _ = _step(torch.bfloat16, 2, 256, 2, 90, mask=(mask, 1))
    da, db = torch.full_like(mask, float("nan")), torch.full_like(mask, float("nan"))
    st.legacy(None, am=_capi.tp_attn_mask(mask=mask.data_ptr(), mode=1, reserved=0, grad=da.data_ptr()))
    st.sink(None, am=_capi.tp_attn_mask(mask=mask.data_ptr(), mode=1, reserved=0, grad=db.data_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(da).all() and float(da.abs().max()) > 0 and torch.equal(da, db)


def test_dx_multi_with_only_the_mlp_trainable_equals_tp_backward_inputs(bf16_step):
    st, _, g, _ = bf16_step
    da, db = (torch.full_like(st.xm, float("nan")) for _ in range(2))
    full, part = st.buffers(), st.buffers(names=MLP)
    st.legacy(full, ig=_capi.tp_input_grads(dx_multi=da.data_ptr()))
    st.sink(part, ig=_capi.tp_input_grads(dx_multi=db.data_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(da).all() and torch.equal(da, db)
    for n, a, b in zip(NAMES, full, part):
        assert torch.equal(a, g[n]), n                            # (the input gradients change no parameter gradient)
        assert (b is None) if n not in MLP else torch.equal(b, a), n


# ---- 7. determinism (the accumulate case: in test 4) ----------------------------------------------------------------------------
def test_a_frozen_subset_is_deterministic():
    (params, x, xm, w), _ = _full_run(torch.bfloat16, 2, 256, 2)
    a = _train_once(params, x, xm, w, 256, 2, torch.bfloat16, K_BRANCH)
    b = _train_once(params, x, xm, w, 256, 2, torch.bfloat16, K_BRANCH)
    for n in K_BRANCH:
        assert torch.equal(a[n], b[n]), n
