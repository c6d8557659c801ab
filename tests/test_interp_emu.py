"""Interpretability maps on the CPU (fiber emulator): the pixel-gradient and attention-rollout kernels (csrc/interp.h) against float64 torch,
the engine's armed backward (vcad_set_input_grads) against oracle autograd, and the contract that an unarmed backward is unchanged."""
import pytest
import torch

import interp_util as IU
import oputil as U
from oracle import restatement as O
from test_engine_emu import engine_masks
from videocad_amd import lib as L
from videocad_amd import synth


@pytest.fixture
def emu():
    with U.emulated() as e:
        yield e


@pytest.mark.parametrize("fold,dt", [(True, torch.bfloat16), (False, torch.float32), (False, torch.bfloat16), (True, torch.float32)])
def test_patch_grad_kernel(emu, fold, dt):
    IU.check_patch_grad(emu, "cpu", 2, 1, fold, dt)


def test_patch_grad_kernel_frames_view_and_scale(emu):
    """T > 1 frames seen through the loader's [:, :-1] view (batch stride (T + 1) S^2), gradient scale 1024 divided out"""
    IU.check_patch_grad(emu, "cpu", 2, 3, True, torch.bfloat16, scale=1024.0, pad_T=1, seed=3)
    IU.check_patch_grad(emu, "cpu", 1, 2, False, torch.float32, scale=4.0, pad_T=1, seed=4)


@pytest.mark.parametrize("st,cls", [(0, 0), (1, 0), (2, 0), (1, 1)])     # (the class-token path exists on 16-bit engines only)
def test_rollout_kernel(emu, st, cls):
    IU.check_rollout(emu, "cpu", 2, 2, st, cls, seed=st)


def small_cfg(**over):
    cfg = dict(O.CANONICAL_CONFIG)
    cfg.update(vit_depth=2, num_decoder_layers=1, window_size=2, max_ep_len=16)
    cfg.update(over)
    return cfg


@pytest.mark.parametrize("pa,ps,V", [(True, True, 0), (False, True, 0), (True, True, 2)])
def test_engine_pixel_grads_match_oracle(emu, pa, ps, V):
    """frame, CAD and multiview pixel gradients of an armed f32 backward against oracle autograd (canonical, states-only and multiview wirings)"""
    cfg = small_cfg(enable_past_actions=pa, enable_past_states=ps, num_views=V)
    eng, weights = IU.build_engine(cfg, L.VCAD_F32)
    B, T = 2, 2
    batch = synth.make_batch(B, T, seed=21, num_views=V) if V else synth.make_batch(B, T, seed=21)
    dcmds, dpars = IU.upstream(B, T, cfg)
    ofr, ocad, omv = IU.oracle_input_grads(weights, cfg, batch, dcmds, dpars)
    efr, ecad, emv = IU.engine_input_grads(eng, cfg, batch, dcmds, dpars)
    assert U.relerr(efr, ofr) < 1e-4, U.relerr(efr, ofr)
    assert U.relerr(ecad, ocad) < 1e-4, U.relerr(ecad, ocad)
    if V:
        assert U.relerr(emv, omv) < 1e-4, U.relerr(emv, omv)
    assert float(ocad.norm()) > 0 and float(ofr.norm()) > 0


def test_engine_pixel_grads_train_mode(emu):
    """dropout on: the oracle is fed the engine's masks; the pixel gradients see every mask the backward applies (emb_dropout included)"""
    cfg = small_cfg()
    eng, weights = IU.build_engine(cfg, L.VCAD_F32)
    B, T = 1, 2
    eng.set_dropout(0.1, seed=4321)
    batch = synth.make_batch(B, T, seed=22)
    dcmds, dpars = IU.upstream(B, T, cfg, seed=1)
    ofr, ocad, _ = IU.oracle_input_grads(weights, cfg, batch, dcmds, dpars, masks=engine_masks(eng, cfg, B, T))
    efr, ecad, _ = IU.engine_input_grads(eng, cfg, batch, dcmds, dpars)
    assert U.relerr(efr, ofr) < 1e-4 and U.relerr(ecad, ocad) < 1e-4, (U.relerr(efr, ofr), U.relerr(ecad, ocad))


def test_arming_changes_nothing_else(emu):
    """weight gradients bit-identical with and without vcad_set_input_grads, the same GEMM launches; the arming is consumed by one backward;
    refusals: no forward, frames of a wiring without the frame tower"""
    cfg = small_cfg()
    eng, weights = IU.build_engine(cfg, L.VCAD_F32)
    B, T = 1, 2
    batch = synth.make_batch(B, T, seed=23)
    dcmds, dpars = IU.upstream(B, T, cfg, seed=2)
    fams = (L.KERNEL_GEMM_DMA, L.KERNEL_GEMM_REG, L.KERNEL_GEMM_MID, L.KERNEL_GEMM_GROUPED)
    counts = lambda: [eng.kernel_launches(f) for f in fams]
    c0 = counts()
    IU.engine_input_grads(eng, cfg, batch, dcmds, dpars, arm=False)
    g_plain = eng.grads.clone(); c1 = counts()
    efr, ecad, _ = IU.engine_input_grads(eng, cfg, batch, dcmds, dpars, arm=True)
    g_armed = eng.grads.clone(); c2 = counts()
    assert torch.equal(g_plain, g_armed)
    assert [b - a for a, b in zip(c0, c1)] == [b - a for a, b in zip(c1, c2)]
    assert torch.isfinite(efr).all() and torch.isfinite(ecad).all()
    # consumed: the backward after an armed one leaves the buffer alone
    buf = torch.zeros(B, 224, 224)
    eng.set_input_grads(None, buf)
    eng.backward(dcmds, dpars)
    assert float(buf.abs().max()) > 0
    buf.fill_(7.0)
    eng.backward(dcmds, dpars)
    assert bool((buf == 7.0).all())
    assert torch.equal(eng.grads, g_plain)
    # refusals
    eng2, _ = IU.build_engine(small_cfg(enable_past_states=False, enable_past_actions=True), L.VCAD_F32, weights=None)
    with pytest.raises(RuntimeError, match="no forward"):
        eng2.set_input_grads(None, torch.zeros(B, 224, 224))
    b2 = synth.make_batch(B, T, seed=24)
    an = O.normalize_actions(torch.from_numpy(b2["actions"])[:, :-1])
    eng2.forward(torch.from_numpy(b2["frames"])[:, :-1], an, torch.from_numpy(b2["cad_image"]))
    with pytest.raises(RuntimeError, match="frame tower"):
        eng2.set_input_grads(torch.zeros(B, T, 224, 224), None)
    eng2.forward(torch.from_numpy(b2["frames"])[:, :-1].mul(127.5).add(127.5).to(torch.uint8), an,
                 torch.from_numpy(b2["cad_image"]).mul(127.5).add(127.5).to(torch.uint8))
    with pytest.raises(RuntimeError, match="uint8"):
        eng2.set_input_grads(None, torch.zeros(B, 224, 224))


def test_engine_rollout_matches_oracle_attention(emu):
    """vcad_cad_attention_rollout (f32 engine, three ViT layers) against the reference's rollout on the oracle's own attention probabilities"""
    cfg = small_cfg(vit_depth=3)
    eng, weights = IU.build_engine(cfg, L.VCAD_F32)
    cad = torch.from_numpy(synth.make_batch(2, 1, seed=25)["cad_image"])
    out = eng.attention_rollout(cad)
    ref = oracle_rollout(weights, cfg, cad)
    assert float((out.double() - ref).abs().max()) < 1e-5, float((out.double() - ref).abs().max())


def oracle_rollout(weights, cfg, cad):
    """float64 restatement of the reference's hooks: every layer's softmax of the CAD tower, then IU.rollout_ref"""
    Pm = {k: torch.tensor(v, dtype=torch.float64) for k, v in weights.items()}
    pre = "cad_embedding_model."
    probs = []
    orig = torch.Tensor.softmax

    def grab(self, dim=None, **kw):
        out = orig(self, dim=dim, **kw)
        if self.dim() == 4:
            probs.append(out.detach())
        return out
    torch.Tensor.softmax = grab
    try:
        with torch.no_grad():
            O.vit_forward(Pm, pre, cad.double(), cfg)
    finally:
        torch.Tensor.softmax = orig
    return IU.rollout_ref(probs[:-1], probs[-1][:, :, 0])
