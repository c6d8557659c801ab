"""Shared checks of the interpretability maps (csrc/interp.h, vcad_set_input_grads, vcad_cad_attention_rollout): the kernels against float64
torch, the engine's pixel gradients against oracle autograd.  Used by test_interp_emu.py (fiber emulator) and test_interp_gpu.py (MI355X)."""
import torch

import oputil as U
from oracle import restatement as O
from videocad_amd import lib as L
from videocad_amd import synth
from videocad_amd.engine import NativeEngine, make_config

S, PATCH, G = 224, 32, 7
P, P1 = G * G, G * G + 1
ENGINE_KEYS = ("hidden_size", "nhead", "num_decoder_layers", "dim_feedforward", "window_size", "act_dim", "num_classes", "num_params",
               "num_params_values", "max_ep_len", "vit_dim", "vit_depth", "vit_heads", "vit_dim_head", "vit_mlp", "image_size", "patch_size",
               "enable_past_actions", "enable_past_states", "enable_timestep_embedding", "num_views")


def patchify(x):
    """[N, S, S] -> [N P, 1024] ('b c (h p1) (w p2) -> b (h w) (p1 p2 c)', c = 1)"""
    N = x.shape[0]
    return x.reshape(N, G, PATCH, G, PATCH).permute(0, 1, 3, 2, 4).reshape(N * P, PATCH * PATCH)


def check_patch_grad(lib, device, B, T, fold, dt, scale=1.0, pad_T=0, seed=0):
    """patch_grad_kernel against float64 autograd of patchify + LayerNorm(1024) on the same (rounded) upstream gradient.  The frames are the
    [:, :T] view of a [B, T + pad_T] batch (the loader's [:, :-1] view: batch stride != T S^2)."""
    full = U.rnd((B, T + pad_T, S, S), "cpu", seed=seed)
    x = full[:, :T]
    rows = B * T * P
    gamma = 1.0 + 0.5 * U.rnd((1024,), "cpu", seed=seed + 1)
    dy = U.rnd((rows, 1024), "cpu", seed=seed + 2)
    x64 = x.double().reshape(B * T, S, S).requires_grad_(True)
    pt = patchify(x64)
    mean = pt.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((pt - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
    xh = (pt - mean) * rstd
    stats = torch.cat([mean, rstd], -1).detach().float().contiguous()
    # folded: the kernel is handed the normalised patches' gradient (gamma already applied); unfolded: the LayerNorm output's, plus gamma
    dxh = (dy * gamma if fold else dy).to(dt)
    up = dxh.double() if fold else dxh.double() * gamma.double()
    (xh * up).sum().backward()
    ref = (x64.grad / scale).reshape(B, T, S, S)
    out = torch.zeros(B, T, S, S, device=device)
    fd, dxh_d, gamma_d, stats_d = full.to(device), dxh.to(device), (None if fold else gamma.to(device)), stats.to(device)     # (alive until the kernel ran)
    L.check(lib, lib.vcad_op_patch_grad(0 if dt == torch.float32 else 1, U.ptr(dxh_d), U.ptr(gamma_d), U.ptr(fd), (T + pad_T) * S * S, U.ptr(stats_d),
                                        U.ptr(out), T * S * S, rows, S, PATCH, T, 1.0 / scale, U.stream_of(device)), "patch_grad")
    if device != "cpu":
        torch.cuda.synchronize()
    err = U.relerr(out, ref)
    assert err < 1e-5, ("patch grad", fold, dt, err)
    return err


def _store(x, st):
    """fp32 values -> (storage tensor, the values the kernel reads back)"""
    if st == 0:
        return x.float().contiguous(), x.float()
    if st == 1:
        h = x.to(torch.bfloat16)
        return h.contiguous(), h.float()
    hi = x.to(torch.bfloat16); lo = (x - hi.float()).to(torch.bfloat16)
    words = (hi.view(torch.int16).to(torch.int32) << 16) | (lo.view(torch.int16).to(torch.int32) & 0xFFFF)
    return words.contiguous(), hi.float() + lo.float()


def rollout_ref(probs_full, last_row0):
    """the reference's rollout (trainer.py compute_attention_rollout) on float64 probabilities: probs_full [layers][N, H, P1, P1], last_row0 [N, H, P1]
    (the class-token layer's row 0 — the only row that reaches e0^T A_L ... A_1).  -> [N, P1 - 1]"""
    N = last_row0.shape[0]
    eye = torch.eye(P1, dtype=torch.float64)
    joint = eye.expand(N, P1, P1)
    for pr in probs_full:
        a = pr.mean(1) + eye
        a = a / a.sum(-1, keepdim=True)
        joint = a.bmm(joint)
    a0 = last_row0.mean(1); a0[:, 0] += 1.0
    a0 = a0 / a0.sum(-1, keepdim=True)
    return torch.einsum("nk,nkj->nj", a0, joint)[:, 1:]


def check_rollout(lib, device, N, nfull, st, cls, H=16, seed=0):
    inner = H * 64
    scale = 64 ** -0.5
    qkvs, lses, probs = [], [], []
    for l in range(nfull):
        x = U.rnd((N * P1, 3 * inner), "cpu", seed=seed + 10 * l)
        stor, val = _store(x, st)
        q = val[:, :inner].reshape(N, P1, H, 64).transpose(1, 2).double()
        k = val[:, inner:2 * inner].reshape(N, P1, H, 64).transpose(1, 2).double()
        s = q @ k.transpose(-1, -2) * scale
        lse = torch.logsumexp(s, -1).float().contiguous()          # [N][H][P1]
        qkvs.append(stor.to(device)); lses.append(lse.to(device)); probs.append(torch.softmax(s, -1))
    if cls:
        D = 512
        ha = U.rnd((N * P1, D), "cpu", seed=seed + 101).to(torch.bfloat16)
        g = U.rnd((N, H, D), "cpu", seed=seed + 102, scale=0.05).to(torch.bfloat16)
        s0 = torch.einsum("nhd,njd->nhj", g.double(), ha.double().view(N, P1, D)) * scale
        last_qkv = None; last_st = 1
        ha_d, g_d = ha.to(device), g.to(device)
    else:
        D = 512
        last_st = 0 if st != 1 else 1
        x = U.rnd((N * P1, 3 * inner), "cpu", seed=seed + 201)
        stor, val = _store(x, last_st)
        q0 = val.view(N, P1, 3 * inner)[:, 0, :inner].reshape(N, H, 64).double()
        k = val[:, inner:2 * inner].reshape(N, P1, H, 64).transpose(1, 2).double()
        s0 = torch.einsum("nhd,nhjd->nhj", q0, k) * scale
        last_qkv = stor.to(device); ha_d = g_d = None
    lse_last = torch.logsumexp(s0, -1).float().contiguous().to(device)
    ref = rollout_ref(probs, torch.softmax(s0, -1))
    out = torch.full((N, P1 - 1), float("nan"), device=device)
    import ctypes as C
    qp = (C.c_void_p * max(1, nfull))(*[t.data_ptr() for t in qkvs]); lp = (C.c_void_p * max(1, nfull))(*[t.data_ptr() for t in lses])
    L.check(lib, lib.vcad_op_attention_rollout(st, qp, lp, nfull, int(cls), U.ptr(last_qkv), last_st, U.ptr(lse_last), U.ptr(ha_d), U.ptr(g_d),
                                               N, H, P1, D, scale, U.ptr(out), U.stream_of(device)), "attention_rollout")
    if device != "cpu":
        torch.cuda.synchronize()
    err = float((out.double().cpu() - ref).abs().max())
    assert err < 1e-5, ("rollout", st, cls, err)
    return err


# ------------------------------------------------------------------------------------------------ engine
def build_engine(cfg, dtype, device="cpu", weights=None):
    shapes = O.param_shapes(cfg)
    if weights is None:
        weights = {k: synth.make_param(k, s) for k, s in shapes.items()}
    eng = NativeEngine(make_config(dtype=dtype, **{k: cfg[k] for k in ENGINE_KEYS if k in cfg}), device)
    for k, w in weights.items():
        eng.view(k).copy_(torch.from_numpy(w))
    eng.sync_shadow()
    return eng, weights


def oracle_input_grads(weights, cfg, batch, dcmds, dpars, masks=None):
    """float32 oracle autograd: gradients of <cmds, dcmds> + <pars, dpars> with respect to frames[:, :-1], cad and the multiview images"""
    Pm = {k: torch.tensor(v, dtype=torch.float32) for k, v in weights.items()}
    frames = torch.from_numpy(batch["frames"])[:, :-1].clone().requires_grad_(True)
    cad = torch.from_numpy(batch["cad_image"]).clone().requires_grad_(True)
    mv = batch.get("multiview_images", None)
    mv = torch.from_numpy(mv).clone().requires_grad_(True) if mv is not None else None
    an = O.normalize_actions(torch.from_numpy(batch["actions"])[:, :-1])
    cmds, pars = O.model_forward(Pm, frames, an, cad, cfg, None, masks, mv)
    ((cmds * dcmds).sum() + (pars.reshape(dpars.shape) * dpars).sum()).backward()
    return frames.grad, cad.grad, (mv.grad if mv is not None else None)


def engine_input_grads(eng, cfg, batch, dcmds, dpars, arm=True):
    """engine forward on the [:, :-1] view, armed backward; -> (dframes [B,T,1,S,S] or None, dcad [B,1,S,S], dmv or None)"""
    dev = eng.device
    frames = torch.from_numpy(batch["frames"]).to(dev); cad = torch.from_numpy(batch["cad_image"]).to(dev)
    an = O.normalize_actions(torch.from_numpy(batch["actions"])[:, :-1]).to(dev)
    mv = batch.get("multiview_images", None)
    mv = torch.from_numpy(mv).to(dev) if mv is not None else None
    B, T = an.shape[:2]
    V = cfg.get("num_views", 0)
    eng.forward(frames[:, :-1], an, cad, mv)
    dfr = torch.full((B, T, S, S), float("nan"), device=dev) if cfg.get("enable_past_states", True) else None
    dcad = torch.full((B * (1 + V), S, S), float("nan"), device=dev)
    if arm:
        eng.set_input_grads(dfr, dcad)
    eng.backward(dcmds.to(dev), dpars.to(dev))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return (dfr.view(B, T, 1, S, S).cpu() if dfr is not None else None, dcad[:B].view(B, 1, S, S).cpu(),
            dcad[B:].view(B, V, 1, S, S).cpu() if V else None)


def upstream(B, T, cfg, seed=0):
    return U.rnd((B, T, cfg["num_classes"]), "cpu", seed=seed + 7), U.rnd((B, T, cfg["num_params"] * cfg["num_params_values"]), "cpu", seed=seed + 8, scale=0.01)
