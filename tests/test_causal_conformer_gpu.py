"""The causal depthwise convolution (`encoder.depthwise_conv_causal`) on the GPU, offline:
  * the three causal kernel entry points against the fp64 references of tests/causal_conformer_ref.py, with the buffers, bounds
    and call patterns of tests/test_convmodule_kernels.py (its `_conv_case` runs here with the causal entry points and references
    in place of the symmetric ones);
  * the causal forward against the SYMMETRIC entry point on an input with (KW-1)/2 zero rows in front of every utterance, bit for
    bit: the same taps in the same order, measured against code this option does not touch;
  * the native layer runtime and the stack call against the per-kernel composition;
  * the offline causal encoder (chunk mask cs 4, L 1) against the bf16-emulating oracle with the causal convolution module."""
import pytest
import torch

from tests import causal_conformer_ref as CR
from tests import convmodule_ref as R
from tests import gpu_checks as G
from tests import test_convmodule_kernels as T
from tests.test_convmodule_kernels import BF, inp, out

pytestmark = pytest.mark.gpu
DEV = G.DEV


@pytest.fixture
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from espresso_amd import _lib

    return _lib.lib()


class _CausalEntryPoints:
    """the library with the causal entry points under their symmetric twins' names (same argument lists)"""

    def __init__(self, lib):
        self.ea_glu_dwconv_fwd = lib.ea_glu_dwconv_causal_fwd
        self.ea_glu_dwconv_bwd = lib.ea_glu_dwconv_causal_bwd
        self.ea_dwconv_bwd_weight = lib.ea_dwconv_causal_bwd_weight
        self.ea_dwconv_wgrad_workspace_bytes = lib.ea_dwconv_wgrad_workspace_bytes


def _causal_conv_case(lib, monkeypatch, B, T_, C, KW, seed=0, dw_prefill=False):
    """test_convmodule_kernels._conv_case: U one ulp; Z, dY ulp + KW 2^-23 sum|terms|; dw M 2^-24 sum|terms| with the one-row
    check; data-only + weight-only calls == the combined call.
    dw_prefill: the gradient is added onto random values, as that file does at T = 129 only.  The bound counts the M = B*T
    products; the one fp32 addition onto a pre-filled dw of magnitude ~1 rounds by up to 2^-24 |dw|, which M 2^-24 sum|terms|
    covers at M = 387 and not at M = 3 (T = 1 with a pre-filled dw: |diff| 6.0e-8 = half an ulp of 1.08 against a bound of
    3.8e-8) — so the time-tile cases accumulate onto zeros, where that addition is exact."""
    for name in ("dwconv", "glu_dwconv_bwd", "dwconv_wgrad"):
        monkeypatch.setattr(R, name, getattr(CR, name))
    return T._conv_case(_CausalEntryPoints(lib), B, T_, C, KW, seed=seed, dw_prefill=dw_prefill)


# ---- G1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KW", [3, 7, 15, 31])
def test_causal_kernels_every_filter_width(lib, monkeypatch, KW):
    _causal_conv_case(lib, monkeypatch, 3, 129, 64, KW, dw_prefill=True)  # (onto a pre-filled dw)


@pytest.mark.parametrize("C", [64, 72])
@pytest.mark.parametrize("T_", [1, 5, 30, 31, 32, 64, 65])  # below, at and past the KW-1 halo; around the 64-step tile
def test_causal_kernels_time_tile_edges(lib, monkeypatch, T_, C):
    _causal_conv_case(lib, monkeypatch, 3, T_, C, 31, seed=7)


def test_causal_kernels_scalar_path(lib, monkeypatch):
    _causal_conv_case(lib, monkeypatch, 3, 65, 66, 7, seed=7)


def test_reference_substitution_is_what_makes_the_case_pass(lib):
    """control: the causal entry points against the SYMMETRIC references fail — the case above tests the padding, not only U"""
    with pytest.raises(AssertionError):
        T._conv_case(_CausalEntryPoints(lib), 3, 65, 64, 7, seed=7)


# ---- G2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 66])
@pytest.mark.parametrize("KW", [31, 7])
def test_causal_forward_equals_symmetric_kernel_on_left_padded_input(lib, KW, C):
    B, T_, PAD = 3, 70, (KW - 1) // 2
    g = T._gen(5 + KW + C)
    Y, w = T._utts(g, B, T_, 2 * C), (torch.randn(C, KW, generator=g) / KW ** 0.5).float()
    Tp = T_ + PAD
    Yp = torch.zeros(B, Tp, 2 * C, dtype=BF)
    Yp[:, PAD:] = Y.view(B, T_, 2 * C)
    bw = inp(w)
    bY, bU, bZ = inp(Y), out((B * T_, C), BF), out((B * T_, C), BF)
    bYp, bUp, bZp = inp(Yp.view(B * Tp, 2 * C)), out((B * Tp, C), BF), out((B * Tp, C), BF)
    assert lib.ea_glu_dwconv_causal_fwd(bY.p, bw.p, bU.p, bZ.p, None, B, T_, C, KW, T._st()) == 0
    assert lib.ea_glu_dwconv_fwd(bYp.p, bw.p, bUp.p, bZp.p, None, B, Tp, C, KW, T._st()) == 0
    torch.cuda.synchronize()
    for o in (bU, bZ, bUp, bZp):
        assert o.intact()
    assert torch.equal(bUp.bits().view(B, Tp, C)[:, PAD:], bU.bits().view(B, T_, C))
    assert torch.equal(bZp.bits().view(B, Tp, C)[:, :T_], bZ.bits().view(B, T_, C)), "causal Z != symmetric Z of the left-padded input"
    assert bool((bZ.cpu().float().abs() > 0).any())


# ---- G4 ----------------------------------------------------------------------------------------------------------------------
def _tiny_causal_model(embed_dim=64, heads=4, ffn=128, cs=0, L=0, causal=True):
    from espresso_amd.models.transformer.speech_transformer_config import SpeechTransformerConfig
    from espresso_amd.models.transformer.speech_transformer_encoder_model import SpeechTransformerEncoderModel

    cfg = SpeechTransformerConfig()
    e = cfg.encoder
    e.embed_dim, e.ffn_embed_dim, e.layers, e.attention_heads = embed_dim, ffn, 2, heads
    e.normalize_before, e.relative_positional_embeddings, e.layer_type = True, True, "conformer"
    e.depthwise_conv_causal = causal
    e.conv_channels = "[64, 64, 16, 16]"
    e.chunk_size, e.chunk_left_window, e.chunk_right_window = cs, L, 0
    cfg.dropout = cfg.attention_dropout = cfg.activation_dropout = 0.0
    cfg.layernorm_embedding = True
    cfg.max_source_positions, cfg.max_target_positions = 3600, 200
    return SpeechTransformerEncoderModel.build_model(cfg, G._Task(40))


def _worst(ga, gb):
    worst = ("", 0.0)
    for n in ga:
        if n.endswith("k_proj.bias") or ("pre_encoder.convolutions." in n and n.endswith(".bias")):
            continue  # exactly zero in exact arithmetic: only rounding noise to compare
        e = float((ga[n] - gb[n]).abs().max() / (ga[n].abs().max() + 1e-6))
        if e > worst[1]:
            worst = (n, e)
    return worst


def test_native_layer_runtime_matches_kernel_composition_causal():
    """gpu_checks.check_native_layer for a layer with the option set (C 64, heads 4, T 37), same bounds: output < 1e-6, worst
    gradient < 2e-3 — and the option is seen by both paths (the symmetric layer's output is far away)"""
    from espresso_amd.modules.conformer_layer import ConformerWithRelativePositionalEmbeddingEncoderLayer as Layer

    C, T_, B = 64, 37, 3
    torch.manual_seed(0)
    model = _tiny_causal_model().to(DEV)
    layer = model.encoder.layers[0]
    assert layer.conv_module.causal
    with torch.no_grad():
        layer.self_attn.pos_bias_u.normal_(0, 0.1)
        layer.self_attn.pos_bias_v.normal_(0, 0.1)
    x0 = G.bf(torch.randn(B * T_, C)).to(DEV)
    key_len = torch.tensor([T_, T_ - 7, max(1, T_ // 3)], dtype=torch.int32, device=DEV)
    model.train()
    outs, grads = [], []
    try:
        for native, causal in ((False, True), (True, True), (True, False), (False, False)):
            Layer.use_native_runtime = native
            layer.conv_module.causal = causal
            for p in layer.parameters():
                p.grad = None
            layer.conv_module.batch_norm.running_mean.zero_()
            layer.conv_module.batch_norm.running_var.fill_(1.0)
            x = x0.clone().requires_grad_(True)
            y = layer(x, B, T_, key_len=key_len)
            (y.float() * torch.linspace(-1, 1, C, device=DEV)).sum().backward()
            torch.cuda.synchronize()
            outs.append(y.detach().float().cpu())
            g = {n: p.grad.detach().float().cpu().clone() for n, p in layer.named_parameters()}
            g["__x"] = x.grad.float().cpu()
            g["__rm"] = layer.conv_module.batch_norm.running_mean.detach().cpu().clone()
            grads.append(g)
    finally:
        Layer.use_native_runtime = True
        layer.conv_module.causal = True
    r = {"out_abs": float((outs[0] - outs[1]).abs().max()), "worst_grad": _worst(grads[0], grads[1]),
         "causal_vs_symmetric_native": float((outs[1] - outs[2]).abs().max()),
         "causal_vs_symmetric_composition": float((outs[0] - outs[3]).abs().max())}
    print(r)
    assert r["out_abs"] < 1e-6, r
    assert r["worst_grad"][1] < 2e-3, r
    assert r["causal_vs_symmetric_native"] > 0.05 and r["causal_vs_symmetric_composition"] > 0.05, r


def test_stack_call_matches_layer_loop_causal(monkeypatch):
    """one encoder-level training step through conformer_stack_native == the per-layer path, same bounds.  (The stack call needs
    the layers' cached bindings, i.e. parameters and gradients in the trainer's flat buffers.)"""
    from espresso_amd import functional as F
    from espresso_amd.optim.flat import FlatParams

    torch.manual_seed(1)
    model = _tiny_causal_model().to(DEV)
    flat = FlatParams(model, DEV)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(3, 150, 80, generator=gen).to(DEV)
    lengths = torch.tensor([150, 121, 66], device=DEV)
    calls = []
    real = F.conformer_stack_native
    monkeypatch.setattr(F, "conformer_stack_native", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    runs = []
    for stack in (True, False):
        F.set_layer_stack(stack)
        try:
            for m in model.modules():
                if getattr(m, "running_mean", None) is not None:
                    m.running_mean.zero_(); m.running_var.fill_(1.0)
            model.train()
            flat.zero_grad()
            lo = model(feats, lengths)["encoder_out"][0].float()
            (lo * torch.linspace(-1, 1, lo.shape[-1], device=DEV)).sum().backward()
            torch.cuda.synchronize()
            runs.append((lo.detach().cpu(), {n: p.grad.detach().float().cpu().clone() for n, p in model.named_parameters()
                                             if p.grad is not None}, len(calls)))
        finally:
            F.set_layer_stack(True)
    assert runs[0][2] == 1 and runs[1][2] == 1, "the stack call was not taken exactly once (first run only)"
    r = {"out_abs": float((runs[0][0] - runs[1][0]).abs().max()), "worst_grad": _worst(runs[1][1], runs[0][1]), "n": len(runs[0][1])}
    print(r)
    assert r["n"] > 60 and r["out_abs"] < 1e-6 and r["worst_grad"][1] < 2e-3, r


# ---- G5 ----------------------------------------------------------------------------------------------------------------------
def test_offline_causal_encoder_vs_emulating_oracle():
    """ref_conformer_ctc_tiny's weights in a model with depthwise_conv_causal, chunk_size 4, chunk_left_window 1 (the masked
    Conformer pass) against oracle.torch_ref.encoder under bf16 emulation with the causal convolution module and chunk_attn_mask;
    test_gpu_parity's bounds for this fixture."""
    from espresso_amd import functional as F
    from oracle import torch_ref

    g, sd, _, _ = G.load_fixture("ref_conformer_ctc_tiny")
    H, cs, L = 4, 4, 1
    model = _tiny_causal_model(cs=cs, L=L).to(DEV)
    G.load_ref_state(model, sd)
    feats_c, lengths_c = torch.from_numpy(g["feats"]), torch.from_numpy(g["lengths"])
    feats, lengths = feats_c.to(DEV), lengths_c.to(DEV)
    ol = torch.from_numpy(g["out::out_lengths"]).long()
    mask = lambda training: torch_ref.chunk_attn_mask(ol, cs, L, 0, training)
    model.eval()
    with torch.no_grad():
        lo = model(feats, lengths)["encoder_out"][0].float().cpu()
    with torch.no_grad(), torch_ref.bf16_emulation(True, flash=False), CR.causal_oracle():
        emu_eval, _ = torch_ref.encoder(feats_c, lengths_c, sd, H=H, layer_type="conformer", training=False, attn_mask=mask(False))
    with torch.no_grad():  # (outside causal_oracle: the symmetric module)
        sym, _ = torch_ref.encoder(feats_c, lengths_c, sd, H=H, layer_type="conformer", training=False, attn_mask=mask(False))
    r = {"eval_logits_vs_emulation": float((lo - emu_eval).abs().max()), "eval_vs_symmetric_oracle": float((lo - sym).abs().max())}
    model.train()
    out_ = model(feats, lengths)
    lt_hip = out_["encoder_out"][0].float().cpu()
    tgt = torch.from_numpy(g["targets"]).to(DEV)
    tl = (tgt != 1).sum(-1)
    B, Tp = out_["encoder_padding_mask"][0].shape
    nll, _ = F.ctc_loss(out_["_logits_bt"][0], tgt.to(torch.int32).contiguous(), out_["src_lengths"][0].to(torch.int32),
                        tl.to(torch.int32), B, Tp, blank=0)
    loss = nll.sum()
    loss.backward()
    torch.cuda.synchronize()
    sde = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and k != "version"
               and not k.endswith("_float_tensor") else v.clone()) for k, v in sd.items()}
    with torch_ref.bf16_emulation(True, flash=False), CR.causal_oracle():
        lt, ole = torch_ref.encoder(feats_c, lengths_c, sde, H=H, layer_type="conformer", training=True, attn_mask=mask(True))
        tg = torch.from_numpy(g["targets"])
        eloss = torch_ref.ctc_loss_sum(lt, tg, ole, (tg != 1).sum(-1))
        eloss.backward()
    r["train_logits_vs_emulation"] = float((lt_hip.detach() - lt.detach()).abs().max())
    r["train_loss"], r["emu_loss"] = float(loss.detach()), float(eloss.detach())
    errs = G._grad_errors(model.encoder.named_parameters(), sde, skip=G._skip_zero_grad_params)
    r["worst_grad_vs_emulation"] = (errs[0][1], errs[0][0])
    r["median_grad_vs_emulation"] = errs[len(errs) // 2][0]
    r["n_grads"] = len(errs)
    print(r)
    assert r["n_grads"] > 60, r
    assert r["eval_vs_symmetric_oracle"] > 0.1, r  # control: the option reaches the offline pass
    assert r["eval_logits_vs_emulation"] < 3.2e-2 and r["train_logits_vs_emulation"] < 4e-2, r
    assert abs(r["train_loss"] - r["emu_loss"]) / r["emu_loss"] < 2e-3, r
    assert r["worst_grad_vs_emulation"][1] < 8e-2 and r["median_grad_vs_emulation"] < 1.2e-2, r
