"""GPU tests of global-norm gradient clipping (csrc/train_kernels.hip plx_gradnorm_* and the *_clip optimizer entry
points; ops/optim.py ``max_grad_norm``) on a real MI355X."""
import pytest
import torch

from polyaxon_amd.ops import _native

pytestmark = pytest.mark.gpu

# Relative tolerance of the measured norm.  A sum of non-negative terms with k fp32 roundings on any path is off by
# at most k * 2^-24; at the sizes below a sensible kernel has k <= 128 (a few elements per thread, the 6-level wave
# tree, the LDS step): 7.6e-6 on the sum of squares, half that on the norm (the finalize is fp64).  2e-5 leaves ~5x.
NORM_RTOL = 2e-5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _measure(lib, ranges, max_norm, dev, state=None):
    """partials over every (tensor) range into disjoint slots + finalize; returns the 4-float device state."""
    slots = [lib.plx_gradnorm_blocks(t.numel()) for t in ranges]
    partials = torch.full((sum(slots),), float("nan"), device=dev)  # every slot must be written
    hp = torch.zeros(8, device=dev)
    hp[5] = max_norm
    state = torch.zeros(4, device=dev) if state is None else state
    first = 0
    for t, k in zip(ranges, slots):
        _native.check(lib.plx_gradnorm_partials(t.data_ptr(), int(t.dtype == torch.bfloat16), t.numel(),
                                                partials.data_ptr() + 4 * first, _stream()), "gradnorm_partials")
        first += k
    _native.check(lib.plx_gradnorm_finalize(partials.data_ptr(), first, hp.data_ptr(), state.data_ptr(), _stream()),
                  "gradnorm_finalize")
    return state


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("dtype,n,offset", [
    *[(torch.float32, n, 0) for n in (4, 8, 12, 1020, 1028, 65540)],
    (torch.float32, 2_097_160, 0),   # past a single pass of the 2048 x 256 float4 grid: the grid-stride loop runs
    *[(torch.bfloat16, n, 0) for n in (4, 8, 12, 1020, 1028, 65540)],   # n % 8 == 4: a 4-element tail
    (torch.bfloat16, 1028, 4),       # 8-B aligned start, n % 8 == 4: a 4-element head, then whole 16-B vectors
    (torch.bfloat16, 1032, 4),       # 8-B aligned start, n % 8 == 0: a head and a tail
    (torch.bfloat16, 4, 4),          # the head alone
])
def test_gradnorm_matches_fp64_norm(cuda, dtype, n, offset):
    lib = _native.lib("plx_train")
    g = torch.Generator(device=cuda).manual_seed(n + offset)
    buf = (torch.randn(n + offset + 8, device=cuda, generator=g) * 3).to(dtype)
    assert buf.data_ptr() % 16 == 0
    t = buf[offset: offset + n]
    assert lib.plx_gradnorm_blocks(n) == min(2048, max(1, (n // 4 + 255) // 256))
    st = _measure(lib, [t], 0.0, cuda)
    torch.cuda.synchronize()
    ref = float(t.double().norm())
    got = st.tolist()
    print(f"dtype={dtype} n={n} offset={offset} norm={got[0]!r} ref={ref!r} rel={_rel(got[0], ref):.3e}")
    assert _rel(got[0], ref) <= NORM_RTOL
    assert got[1] == 1.0 and got[2] == 0.0 and got[3] == 0.0  # max_norm <= 0: scale exactly 1, the norm still measured


def test_gradnorm_two_ranges_scale_and_non_finite(cuda):
    """lp-mode shape of the pass: a bf16 range and an fp32 range into disjoint slots; the scale is
    clip_grad_norm_'s; a non-finite norm publishes scale 0 / skip 1 and counts the skipped step."""
    lib = _native.lib("plx_train")
    a = torch.randn(4100, device=cuda).to(torch.bfloat16)
    b = torch.randn(260, device=cuda)
    ref = float(torch.cat([a.float(), b]).double().norm())
    st = _measure(lib, [a, b], 0.25 * ref, cuda)
    got = st.tolist()
    assert _rel(got[0], ref) <= NORM_RTOL
    want = torch.tensor(0.25 * ref, dtype=torch.float32) / (torch.tensor(got[0], dtype=torch.float32) + 1e-6)
    # an fp32 add and an fp32 divide of the published norm: within a few 2^-24 of the same formula on the host
    assert got[1] == pytest.approx(float(want), rel=1e-6) and got[1] < 1.0 and got[2:] == [0.0, 0.0]
    st = _measure(lib, [a, b], 1e9, cuda, state=st)
    assert st.tolist()[1] == 1.0
    for bad, where in ((float("inf"), a), (float("nan"), b), (3e38, b)):  # 3e38^2 overflows fp32: non-finite too
        keep = where[3].clone()
        where[3] = bad
        st = _measure(lib, [a, b], 1.0, cuda, state=st)
        where[3] = keep
        got = st.tolist()
        assert got[1] == 0.0 and got[3] == 1.0 and not torch.isfinite(torch.tensor(got[0]))
    assert st.tolist()[2] == 3.0
    st = _measure(lib, [a, b], 1.0, cuda, state=st)  # a clean step clears the skip flag, keeps the count
    assert st.tolist()[2:] == [3.0, 0.0]


def test_gradnorm_is_deterministic_and_ignores_the_adamw_grid_cap(cuda):
    lib = _native.lib("plx_train")
    bufs = [torch.randn(2_097_160, device=cuda), torch.randn(65540, device=cuda).to(torch.bfloat16)]
    try:
        for t in bufs:
            first = _measure(lib, [t], 0.0, cuda)[0].clone()
            again = _measure(lib, [t], 0.0, cuda)[0].clone()
            lib.plx_set_adamw_grid_cap(32)
            capped = _measure(lib, [t], 0.0, cuda)[0].clone()
            lib.plx_set_adamw_grid_cap(2048)
            assert lib.plx_gradnorm_blocks(t.numel()) == min(2048, (t.numel() // 4 + 255) // 256)
            torch.cuda.synchronize()
            assert first.view(torch.int32).item() == again.view(torch.int32).item() == capped.view(torch.int32).item()
    finally:
        lib.plx_set_adamw_grid_cap(2048)  # the library default


def _clip_state(lib, grads, dev, frac=0.25):
    """The state the clip kernels read, from a threshold below the norm (scale < 1)."""
    ref = float(torch.cat([g.float().reshape(-1) for g in grads]).double().norm())
    st = _measure(lib, grads, frac * ref, dev)
    scale = st.tolist()[1]
    assert 0.0 < scale < 1.0
    return st, scale


def test_adamw_flat_clip_matches_torch(cuda):
    lib = _native.lib("plx_train")
    n, n_decay = 8192 + 4, 4096
    p = torch.randn(n, device=cuda)
    m = torch.zeros(n, device=cuda)
    v = torch.zeros(n, device=cuda)
    hp = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.01, 0, 0, 0], device=cuda)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    pa = torch.nn.Parameter(p[:n_decay].clone())
    pb = torch.nn.Parameter(p[n_decay:].clone())
    opt = torch.optim.AdamW([{"params": [pa], "weight_decay": 0.01}, {"params": [pb], "weight_decay": 0.0}],
                            lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for it in range(3):
        grad = torch.randn(n, device=cuda)
        g = grad.clone()
        st, scale = _clip_state(lib, [g], cuda)
        _native.check(lib.plx_adamw_flat_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, n_decay,
                                              hp.data_ptr(), step.data_ptr(), st.data_ptr(), _stream()), "adamw_clip")
        step += 1
        scaled = grad * scale  # the torch update fed the scale the kernel published
        pa.grad, pb.grad = scaled[:n_decay].clone(), scaled[n_decay:].clone()
        opt.step()
        assert float(g.abs().max()) == 0.0
    torch.cuda.synchronize()
    torch.testing.assert_close(p, torch.cat([pa.detach(), pb.detach()]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("n", [4, 12, 4100, 4104])
def test_adamw_mixed_clip_matches_torch(cuda, n, wide):
    """n % 8 == 4 runs the 4-wide kernel whatever the knob says; n = 4104 with the knob on runs the 8-wide
    non-temporal one, and both give bitwise the same update (the scaled gradient is an explicit fp32 value)."""
    lib = _native.lib("plx_train")
    res = {}
    try:
        for w in sorted({0, wide}):
            lib.plx_set_adamw_wide(w)
            gen = torch.Generator(device=cuda).manual_seed(n)
            p = torch.randn(n, device=cuda, generator=gen)
            m = torch.zeros(n, device=cuda)
            v = torch.zeros(n, device=cuda)
            plp = torch.empty(n, dtype=torch.bfloat16, device=cuda)
            hp = torch.tensor([1e-3, 0.9, 0.95, 1e-8, 0.1, 0, 0, 0], device=cuda)
            step = torch.zeros(1, dtype=torch.int32, device=cuda)
            pa = torch.nn.Parameter(p.clone())
            opt = torch.optim.AdamW([pa], lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
            for it in range(3):
                g = torch.randn(n, device=cuda, generator=gen).to(torch.bfloat16)
                grad = g.float()
                st, scale = _clip_state(lib, [g], cuda)
                _native.check(lib.plx_adamw_mixed_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                       plp.data_ptr(), n, 1, hp.data_ptr(), step.data_ptr(),
                                                       st.data_ptr(), _stream()), "adamw_mixed_clip")
                step += 1
                pa.grad = grad * scale
                opt.step()
                assert float(g.float().abs().max()) == 0.0
            torch.cuda.synchronize()
            torch.testing.assert_close(p, pa.detach(), rtol=1e-5, atol=1e-6)
            assert torch.equal(plp, p.to(torch.bfloat16))
            res[w] = (p.clone(), m.clone(), v.clone())
    finally:
        lib.plx_set_adamw_wide(0)  # the library default
    if wide:
        for a, b in zip(res[0], res[wide]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("nesterov", [0.0, 1.0])
def test_sgd_flat_clip_matches_reference(cuda, first, nesterov):
    lib = _native.lib("plx_train")
    n, n_decay = 4096 * 3 + 4, 4096 * 2
    p = torch.randn(n, device=cuda)
    g = torch.randn(n, device=cuda)
    m = torch.randn(n, device=cuda)
    hp = torch.tensor([0.1, 0.9, 1e-3, nesterov, 0.1, 0, 0, 0], device=cuda)
    step = torch.tensor([first], dtype=torch.int32, device=cuda)
    st, scale = _clip_state(lib, [g], cuda)
    pr, mr = p.clone(), m.clone()
    gr = g * scale  # torch's order: clip, then weight decay
    gr[:n_decay] += 1e-3 * pr[:n_decay]
    mr = gr.clone() if first == 0 else 0.9 * mr + 0.9 * gr
    d = gr + 0.9 * mr if nesterov else mr
    pr = pr - 0.1 * d
    _native.check(lib.plx_sgd_flat_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), n, n_decay, hp.data_ptr(),
                                        step.data_ptr(), st.data_ptr(), _stream()), "sgd_clip")
    torch.cuda.synchronize()
    torch.testing.assert_close(p, pr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m, mr, rtol=1e-5, atol=1e-6)
    assert float(g.abs().max()) == 0.0


# ---------------------------------------------------------------- the optimizer on the 2-layer GPT-2 (lp mode)
def _gpt2(cuda, max_grad_norm):
    from polyaxon_amd.models.transformer import Transformer, gpt2_125m
    from polyaxon_amd.ops.flat import FlatParams
    from polyaxon_amd.ops.optim import FusedAdamW

    torch.manual_seed(0)
    cfg = gpt2_125m(vocab_size=256, n_layers=2, d_model=256, n_heads=2, d_ff=1024, max_seq_len=128)
    with torch.device(cuda):
        model = Transformer(cfg)
    flat = FlatParams(model, cuda, channels_last=False, lp_dtype=torch.bfloat16)
    flat.enable_direct_grads(True)
    return model, flat, FusedAdamW(flat, lr=3e-3, weight_decay=0.1, max_grad_norm=max_grad_norm)


def _backward(model, tok):
    from polyaxon_amd.models.transformer import lm_loss

    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = lm_loss(model(tok), tok)
    loss.backward()  # ends with the side-stream join: the flat gradient slots are complete
    return loss


def test_lp_mode_scale_one_is_a_noop_and_grad_norm_end_to_end(cuda):
    """3 steps with max_grad_norm=0.0 are bitwise the 3 steps without clipping (params and the bf16 copy), and
    grad_norm() is the norm of the whole gradient taken just before each step_()."""
    res = {}
    for c in (None, 0.0):
        model, flat, opt = _gpt2(cuda, c)
        gen = torch.Generator(device=cuda).manual_seed(9)
        for _ in range(3):
            tok = torch.randint(0, 256, (2, 128), device=cuda, generator=gen)
            _backward(model, tok)
            if c is not None:
                ref = float(torch.cat([flat.lp_grads.float(), flat.grads]).double().norm())
            opt.step_()
            opt.step += 1
            if c is not None:
                gn = opt.grad_norm()
                assert gn.dim() == 0 and gn.is_cuda
                print(f"grad_norm={float(gn)!r} ref={ref!r} rel={_rel(float(gn), ref):.3e}")
                assert ref > 0 and _rel(float(gn), ref) <= NORM_RTOL
                assert opt.clip_stats()["scale"] == 1.0
        torch.cuda.synchronize()
        res[c] = (flat.params.clone(), flat.lp_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    for a, b in zip(res[None], res[0.0]):
        assert torch.equal(a, b)


def test_lp_mode_non_finite_steps_are_skipped(cuda):
    model, flat, opt = _gpt2(cuda, 1.0)
    gen = torch.Generator(device=cuda).manual_seed(3)

    def tokens():
        return torch.randint(0, 256, (2, 128), device=cuda, generator=gen)

    _backward(model, tokens())
    opt.step_()
    opt.step += 1
    assert opt.clip_stats()["skipped"] == 0
    for i, (buf, bad) in enumerate(((flat.lp_grads, float("inf")), (flat.grads, float("nan")))):
        before = [t.clone() for t in (flat.params, flat.lp_params, opt.exp_avg, opt.exp_avg_sq)]
        _backward(model, tokens())
        buf[5] = bad
        opt.step_()  # (the step counter does not advance on a skipped step here; the kernels never read it then)
        torch.cuda.synchronize()
        for a, b in zip(before, (flat.params, flat.lp_params, opt.exp_avg, opt.exp_avg_sq)):
            assert torch.equal(a, b)
        assert float(flat.lp_grads.float().abs().max()) == 0.0 and float(flat.grads.abs().max()) == 0.0
        st = opt.clip_stats()
        assert st["skipped"] == i + 1 and st["scale"] == 0.0
    p0 = flat.params.clone()
    _backward(model, tokens())
    opt.step_()
    torch.cuda.synchronize()
    st = opt.clip_stats()
    assert st["skipped"] == 2 and 0.0 < st["scale"] <= 1.0
    assert not torch.equal(flat.params, p0) and bool(torch.isfinite(flat.params).all())
    assert torch.equal(flat.lp_params, flat.params[: flat.n_decay].to(torch.bfloat16))


def test_captured_step_clips_with_a_per_trial_threshold(cuda):
    """The clip kernels are ordinary launches with fixed pointers: the mlp program's captured step is accepted, and
    the threshold changes between replays of the same graph."""
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program("mlp", {"clip_grad": True}, cuda)
    ex = prog.executor
    assert "max_grad_norm" in prog.hp_keys and ex.use_graph
    ex.capture(warmup=2)
    assert ex.graph is not None and not ex.graph_rejected
    graph = ex.graph
    ex.reset(seed=1)
    ex.set_hparams(lr=0.01, momentum=0.9, weight_decay=1e-4, max_grad_norm=1e-4)
    ex.run(1)
    st = ex.clip_stats()
    assert 0.0 < st["scale"] < 1.0 and st["grad_norm"] > 1e-4
    assert st["scale"] == pytest.approx(1e-4 / st["grad_norm"], rel=1e-5)
    ex.set_hparams(max_grad_norm=1e4)
    ex.run(1)
    st = ex.clip_stats()
    assert st["scale"] == 1.0 and st["grad_norm"] > 0
    assert ex.graph is graph
    assert float(ex.grad_norm()) == st["grad_norm"]
