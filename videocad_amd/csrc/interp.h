// interp.h — the two analysis kernels behind the trainer's interpretability maps (reference trainer.py generate_saliency_batch /
// compute_attention_rollout): the pixel gradient of the patch embedding's LayerNorm(1024), and the CAD tower's attention rollout.
// Neither is on the training path: the engine launches the first only when vcad_set_input_grads armed a backward, the second
// only from vcad_cad_attention_rollout.  Included by ops_misc.hip only.
#pragma once
#include "ops.h"

// ---- pixel gradient of Rearrange -> LayerNorm(1024).  dxh = gradient w.r.t. the NORMALISED patch (x - mean) rstd, i.e. the LayerNorm output's gradient times
// gamma: the caller passes gamma when dxh is still the gradient of the affine output (unfolded patch embedding), or nullptr when gamma is already folded in
// (16-bit engines: dxh = dpe . 16-bit(W diag gamma)).  x-hat is recomputed from the pixels and the forward's (mean, rstd), the way patch_load read them.
//     dx = rstd (dxh - mean(dxh) - xhat mean(dxh xhat)) / grad_scale,  written straight into image layout [n][ph 32 + p1][pw 32 + p2].
// One wave per patch row (VPL = 16, the ln_bwd_kernel shape); lane l holds columns g 256 + 4 l .. +3, so eight lanes cover one 32-pixel patch row: every
// store instruction writes whole 128-byte pieces of image rows.
// (PatchGradParams: ops.h)
template <typename TD, int VPL>
VC_KERNEL __launch_bounds__(256) void patch_grad_kernel(PatchGradParams p) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    constexpr int C = 64 * VPL;
    if (row >= p.rows) return;
    float x[VPL], d[VPL];
    patch_load<VPL>(p.x, 0, row, x, lane, p.img, p.patch, p.T, p.ldx);
    row_load<TD, VPL>((const TD*)p.dxh + row * p.lddxh, d, lane);
    if (p.gamma) {
        float g[VPL];
        row_load<float, VPL>(p.gamma, g, lane);
#pragma unroll
        for (int i = 0; i < VPL; ++i) d[i] *= g[i];
    }
    const float mean = p.stats[row * 2], rstd = p.stats[row * 2 + 1];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) { x[i] = (x[i] - mean) * rstd; c1 += d[i]; c2 += d[i] * x[i]; }
    c1 = vc_wave_sum(c1) * (1.0f / C); c2 = vc_wave_sum(c2) * (1.0f / C);
    const float k = rstd * p.inv_scale;
#pragma unroll
    for (int i = 0; i < VPL; ++i) d[i] = k * (d[i] - c1 - x[i] * c2);
    const int g_ = p.img / p.patch;
    const long n = row / (g_ * g_);
    const int pp = (int)(row % (g_ * g_)), ph = pp / g_, pw = pp % g_;
    float* o = p.out + (n / p.T) * p.ldo + (n % p.T) * (long)p.img * p.img + (long)(ph * p.patch) * p.img + pw * p.patch;
#pragma unroll
    for (int g = 0; g < VPL / 4; ++g) {
        const int e = g * 256 + lane * 4;
        quad_store<float>(o + (long)(e / p.patch) * p.img + e % p.patch, &d[g * 4]);
    }
}

// ---- attention rollout of one ViT tower (Abnar & Zuidema 2020, in the reference's form): per layer A = mean_heads(softmax) + I, row-normalised by its actual
// row sums; joint = A_L ... A_1; the map is row 0 of joint over the patch tokens.  The probabilities are recomputed from what the forward saved — every full
// layer's qkv [N P1][3 inner] (16-bit, fp32, or bf16x3 pre-split words) and lse [N][H][P1] — as p = exp(scale q.k - lse).  The last layer is class-token-only
// and only row 0 of its A is needed (e0^T A_L ... A_1): its probabilities come from the class row's query and the keys of all tokens in qkv, or, on the
// re-associated class-token path (attn_cls.h), from p_j = exp(scale g_h . h_j - lse[N][H]).
// One workgroup per image; the P1 x P1 joint matrix stays in LDS; each thread keeps its entries of the head-summed A in registers.
// (RolloutParams, RO_*: ops.h)
template <typename T> VC_DEV float ro_ld(const void* p, long i) { return vc_ld((const T*)p + i); }
VC_DEV float ro_ldst(int st, const void* p, long i) {
    return st == 0 ? ro_ld<float>(p, i) : (st == 1 ? ro_ld<vc_bf16>(p, i) : ro_ld<vc_pk>(p, i));
}
VC_KERNEL __launch_bounds__(256) void attn_rollout_kernel(RolloutParams p) {
    VC_SHARED float joint[RO_MAXP * RO_LD];
    VC_SHARED float buf[2 * RO_MAXP * RO_LD];                  // per head: q | k (fp32); after the heads: A | the new joint.  Last layer: g [H][D] (cls path)
    VC_SHARED float rinv[RO_MAXP];
    VC_SHARED float pr[RO_MAXH * RO_MAXP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P1 = p.P1, H = p.H, NE = P1 * P1;
    const long n = blockIdx.x;
    float* qs = buf; float* ks = buf + RO_MAXP * RO_LD;
    for (int e = tid; e < NE; e += 256) { const int i = e / P1, j = e % P1; joint[i * RO_LD + j] = i == j ? 1.f : 0.f; }
    for (int L = 0; L < p.nfull; ++L) {
        float acc[RO_MAXP * RO_MAXP / 256];
#pragma unroll
        for (int r = 0; r < RO_MAXP * RO_MAXP / 256; ++r) acc[r] = 0.f;
        for (int h = 0; h < H; ++h) {
            vc_sync();
            for (int e = tid; e < P1 * RO_DH; e += 256) {
                const int i = e / RO_DH, d = e % RO_DH;
                const long base = (n * P1 + i) * p.ldqkv + h * RO_DH + d;
                qs[i * RO_LD + d] = ro_ldst(p.st, p.qkv[L], base);
                ks[i * RO_LD + d] = ro_ldst(p.st, p.qkv[L], base + p.inner);
            }
            vc_sync();
            const float* lse = p.lse[L] + (n * H + h) * P1;
#pragma unroll
            for (int r = 0; r < RO_MAXP * RO_MAXP / 256; ++r) {
                const int e = tid + 256 * r;
                if (e < NE) {
                    const int i = e / P1, j = e % P1;
                    float s = 0.f;
                    for (int d = 0; d < RO_DH; ++d) s += qs[i * RO_LD + d] * ks[j * RO_LD + d];
                    acc[r] += expf(s * p.scale - lse[i]);
                }
            }
        }
        vc_sync();
        float* A = qs; float* nj = ks;
#pragma unroll
        for (int r = 0; r < RO_MAXP * RO_MAXP / 256; ++r) {
            const int e = tid + 256 * r;
            if (e < NE) { const int i = e / P1, j = e % P1; A[i * RO_LD + j] = acc[r] / (float)H + (i == j ? 1.f : 0.f); }
        }
        vc_sync();
        if (tid < P1) { float s = 0.f; for (int j = 0; j < P1; ++j) s += A[tid * RO_LD + j]; rinv[tid] = 1.f / s; }
        vc_sync();
        for (int e = tid; e < NE; e += 256) {
            const int i = e / P1, j = e % P1;
            float s = 0.f;
            for (int k = 0; k < P1; ++k) s += A[i * RO_LD + k] * joint[k * RO_LD + j];
            nj[i * RO_LD + j] = s * rinv[i];
        }
        vc_sync();
        for (int e = tid; e < NE; e += 256) { const int i = e / P1, j = e % P1; joint[i * RO_LD + j] = nj[i * RO_LD + j]; }
    }
    vc_sync();
    // last layer, class row: pr[h][j] = p_h(0 -> j)
    if (p.cls) {
        for (int e = tid; e < H * p.D; e += 256) buf[e] = vc_ld((const vc_bf16*)p.g + n * H * p.D + e);
        vc_sync();
        for (int j = wave; j < P1; j += 4) {                    // wave = token, lanes split D (coalesced row reads)
            const vc_bf16* hj = (const vc_bf16*)p.ha + (n * P1 + j) * p.ldha;
            for (int h = 0; h < H; ++h) {
                float s = 0.f;
                for (int d = lane; d < p.D; d += 64) s += buf[h * p.D + d] * vc_ld(hj + d);
                s = vc_wave_sum(s);
                if (lane == 0) pr[h * RO_MAXP + j] = expf(s * p.scale - p.last_lse[n * H + h]);
            }
        }
    } else {
        for (int e = tid; e < H * P1; e += 256) {
            const int h = e / P1, j = e % P1;
            const long q0 = n * P1 * p.ldqkv + h * RO_DH, k0 = (n * P1 + j) * p.ldqkv + p.inner + h * RO_DH;
            float s = 0.f;
            for (int d = 0; d < RO_DH; ++d) s += ro_ldst(p.last_st, p.last_qkv, q0 + d) * ro_ldst(p.last_st, p.last_qkv, k0 + d);
            pr[h * RO_MAXP + j] = expf(s * p.scale - p.last_lse[n * H + h]);
        }
    }
    vc_sync();
    float* a0 = buf;                                           // row 0 of the last layer's A, then its inverse row sum
    if (tid < P1) { float s = 0.f; for (int h = 0; h < H; ++h) s += pr[h * RO_MAXP + tid]; a0[tid] = s / (float)H + (tid == 0 ? 1.f : 0.f); }
    vc_sync();
    if (tid == 0) { float s = 0.f; for (int j = 0; j < P1; ++j) s += a0[j]; rinv[0] = 1.f / s; }
    vc_sync();
    for (int j = tid + 1; j < P1; j += 256) {
        float s = 0.f;
        for (int k = 0; k < P1; ++k) s += a0[k] * joint[k * RO_LD + j];
        p.out[n * (P1 - 1) + j - 1] = s * rinv[0];
    }
}
