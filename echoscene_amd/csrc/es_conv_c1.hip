// conv_in of the VQ-VAE encoder (Encoder3D, vqvae_modules.py:205-209): one input channel, 3x3x3, padding 1.
#include "es_common.h"

// ---------------------------------------------------------------------------------------------
// k_conv_c1: out[m, n] = bias[n] + sum_t x[src(m, t)] * w[n][t], fp32 FMA over the 27 taps in (kd, kh, kw) order.
// A write-bound kernel (64^3, N = 64: 1 MB in, 67 MB out per object).  Workgroup = one 4 x 4 x 16 block of voxels; its 6 x 6 x 18
// halo'd input sits in LDS (zero outside the volume).  A lane owns ONE group of four output channels for the whole block -- its
// 27 x 4 weights stay in registers -- and walks over the voxels: the NG_ lanes of a voxel read the same LDS words (broadcast) and
// write NG_ x 16 B = one contiguous output row; a wave's 64 / NG_ voxels are consecutive along w, i.e. consecutive rows.
// Output rows are addressed with 64-bit offsets.
// ---------------------------------------------------------------------------------------------
constexpr int C1_TD = 4, C1_TH = 4, C1_TW = 16;
constexpr int C1_HALO = (C1_TD + 2) * (C1_TH + 2) * (C1_TW + 2);

template <int NG_>
__global__ __launch_bounds__(256) void k_conv_c1(const es_conv_c1_args a) {
    __shared__ float tile[C1_HALO];
    __shared__ float wl[NG_ * 4 * 27];
    const int tid = threadIdx.x;
    const int tw = a.W / C1_TW, th = a.H / C1_TH, td = a.D / C1_TD;
    int b = blockIdx.x;
    const int bw = b % tw; b /= tw;
    const int bh = b % th; b /= th;
    const int bd = b % td;
    const int o = b / td;
    const int d0 = bd * C1_TD, h0 = bh * C1_TH, w0 = bw * C1_TW;
    for (int i = tid; i < C1_HALO; i += 256) {
        const int lw = i % (C1_TW + 2), lh = (i / (C1_TW + 2)) % (C1_TH + 2), ld = i / ((C1_TW + 2) * (C1_TH + 2));
        const int d = d0 + ld - 1, h = h0 + lh - 1, w = w0 + lw - 1;
        const bool ok = d >= 0 && d < a.D && h >= 0 && h < a.H && w >= 0 && w < a.W;
        tile[i] = ok ? a.x[(((long)o * a.D + d) * a.H + h) * a.W + w] : 0.0f;
    }
    for (int i = tid; i < NG_ * 4 * 27; i += 256) wl[i] = a.w[i];
    __syncthreads();
    const int cg = tid % NG_, vs = tid / NG_;
    float wr[27][4];
#pragma unroll
    for (int t = 0; t < 27; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) wr[t][c] = wl[(cg * 4 + c) * 27 + t];
    f4 bs = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) bs = *(const f4*)(a.bias + cg * 4);
    constexpr int VP = 256 / NG_;                // voxels per pass
    for (int v = vs; v < C1_TD * C1_TH * C1_TW; v += VP) {
        const int lw = v % C1_TW, lh = (v / C1_TW) % C1_TH, ld = v / (C1_TW * C1_TH);
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float xv = tile[((ld + kd) * (C1_TH + 2) + lh + kh) * (C1_TW + 2) + lw + kw];
                    const int t = (kd * 3 + kh) * 3 + kw;
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = __fmaf_rn(xv, wr[t][c], acc[c]);
                }
        acc += bs;
        const long m = (((long)o * a.D + d0 + ld) * a.H + h0 + lh) * a.W + w0 + lw;
        if (a.out_f32) *(f4*)(a.out_f32 + m * a.N + cg * 4) = acc;
        if (a.out_f16) *(h4*)((_Float16*)a.out_f16 + m * a.N + cg * 4) = h4{(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
    }
}

extern "C" int es_conv_c1_f32(const es_conv_c1_args* a, es_stream stream) {
    ES_REQUIRE(a && a->x && a->w && (a->out_f32 || a->out_f16), "es_conv_c1_f32: NULL argument");
    ES_REQUIRE(a->O > 0 && a->D > 0 && a->H > 0 && a->W > 0 && a->D % C1_TD == 0 && a->H % C1_TH == 0 && a->W % C1_TW == 0,
               "es_conv_c1_f32: O=%d, D,H,W=(%d,%d,%d): D, H multiples of 4, W a multiple of 16", a->O, a->D, a->H, a->W);
    const long nblk = (long)a->O * (a->D / C1_TD) * (a->H / C1_TH) * (a->W / C1_TW);
    ES_REQUIRE(nblk < (1L << 31), "es_conv_c1_f32: too many voxel blocks (%ld)", nblk);
    ES_REQUIRE((((uintptr_t)a->out_f32 | (uintptr_t)a->bias) & 15) == 0 && ((uintptr_t)a->out_f16 & 7) == 0,
               "es_conv_c1_f32: outputs and bias must be 16-byte (f16: 8-byte) aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), blk(256);
    switch (a->N) {
        case 16: hipLaunchKernelGGL(k_conv_c1<4>, grid, blk, 0, st, *a); break;
        case 32: hipLaunchKernelGGL(k_conv_c1<8>, grid, blk, 0, st, *a); break;
        case 64: hipLaunchKernelGGL(k_conv_c1<16>, grid, blk, 0, st, *a); break;
        case 128: hipLaunchKernelGGL(k_conv_c1<32>, grid, blk, 0, st, *a); break;
        default: ES_REQUIRE(false, "es_conv_c1_f32: N=%d output channels (16, 32, 64 or 128)", a->N);
    }
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
