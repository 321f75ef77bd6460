// Shape-preserving sampling (keep given shapes while the others are generated):
//   * k_ddim_blend -- the masked-DDIM blend of DDIMSampler.ddim_sampling (samplers/ddim.py:160-163) with q_sample
//     (echo2shape.py:254-258), planned in front of every step's denoiser;
//   * k_conv_c1    -- conv_in of the VQ-VAE encoder (Encoder3D, vqvae_modules.py:205-209): one input channel, 3x3x3, padding 1.
// Box-preserving sampling (keep given boxes while the others are placed around them):
//   * k_ddpm_update_keep -- the ancestral layout update (p_sample_sg, diffusion_ddpm.py:296-309) that also leaves the kept nodes' rows
//     at the NEXT iteration's q_sample (GaussianDiffusion.q_sample, diffusion_ddpm.py:191-201): the masked loop without a launch of
//     its own in the latency-bound layout step;
//   * k_box_prescale     -- scale_box_params + preprocess_angle2sincos (helpers/util.py:516-540), the inverse of es_box_postprocess.
#include "es_common.h"

// ---------------------------------------------------------------------------------------------
// x[o, :] = mask[o] ? tab[2 st] * x0[o, :] + tab[2 st + 1] * noise[st][o, :] : x[o, :]          (st = *step, not advanced)
// The reference forms q_sample as two products and a sum in fp32 (no fused multiply-add) and blends with a 0 / 1 mask:
// img_orig * 1 + 0 * img is img_orig, img_orig * 0 + 1 * img is img -- so a kept row is the q_sample bits and any other row is
// left alone (neither read nor written).  One lane per 16 bytes, grid.y = object.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ddim_blend(const es_blend_args a) {
#pragma clang fp contract(off)
    const int o = blockIdx.y;
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= a.n || a.mask[o] == 0.0f) return;
    const int st = *a.step;
    const float ca = a.tab[2 * st], cb = a.tab[2 * st + 1];
    const long row = (long)o * a.n + i;
    const f4 v0 = *(const f4*)(a.x0 + row);
    const f4 nz = *(const f4*)(a.noise + (long)st * a.noise_stride + row);
    f4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float p = ca * v0[e], q = cb * nz[e];
        r[e] = p + q;
    }
    *(f4*)(a.x + row) = r;
}

extern "C" int es_ddim_blend(const es_blend_args* a, es_stream stream) {
    ES_REQUIRE(a && a->x && a->x0 && a->mask && a->noise && a->tab && a->step, "es_ddim_blend: NULL argument");
    ES_REQUIRE(a->O > 0 && a->n > 0 && a->n % 4 == 0 && a->noise_stride % 4 == 0 && (long)a->noise_stride >= (long)a->O * a->n,
               "es_ddim_blend: O=%d n=%d noise_stride=%d (n and the stride multiples of 4, stride >= O * n)", a->O, a->n, a->noise_stride);
    ES_REQUIRE(a->O <= 65535, "es_ddim_blend: O=%d objects (<= 65535)", a->O);
    ES_REQUIRE((((uintptr_t)a->x | (uintptr_t)a->x0 | (uintptr_t)a->noise) & 15) == 0, "es_ddim_blend: x, x0 and noise must be 16-byte aligned");
    hipLaunchKernelGGL(k_ddim_blend, dim3((a->n / 4 + 255) / 256, a->O), dim3(256), 0, (hipStream_t)stream, *a);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

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

// ---------------------------------------------------------------------------------------------
// k_ddpm_update_keep: es_ddpm_update's arithmetic on the rows whose mask is 0 (the same expressions in the same order as k_ddpm_update,
// es_rows.hip: the same bits), and on the rows whose mask is 1 the state the denoiser of the NEXT iteration has to see:
//     st + 1 <  n_tab:  x[i] = tab[2 (st+1)] * x0[i] + tab[2 (st+1) + 1] * keep_noise[st+1][i]      (two products, one sum, uncontracted)
//     st + 1 == n_tab:  x[i] = x0[i]                                                                (the loop's result: the caller's bits)
// A kept element reads neither eps nor the step's noise draw, and is never clipped; row st + 1 of tab / keep_noise is only touched
// when it exists.  ONE_BLOCK as k_ddpm_update: the whole state in one workgroup, which advances the step counter itself.
// ---------------------------------------------------------------------------------------------
template <bool ONE_BLOCK>
__global__ void k_ddpm_update_keep(const es_ddpm_keep_args a) {
#pragma clang fp contract(off)
    const int st = *a.step;
    const float* c = a.coef + (long)st * a.coef_stride;
    const bool last = st + 1 >= a.n_tab;
    float ka = 0.0f, kb = 0.0f;
    if (!last) { ka = a.tab[2 * (st + 1)]; kb = a.tab[2 * (st + 1) + 1]; }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += ONE_BLOCK ? (int)blockDim.x : a.n) {
        if (a.mask[i / a.row] != 0.0f) {
            float v = a.x0[i];
            if (!last) {
                const float p = ka * v, q = kb * a.keep_noise[(long)(st + 1) * a.keep_noise_stride + i];
                v = p + q;
            }
            a.x[i] = v;
            continue;
        }
        const float x = a.x[i];
        const int ns = a.eps_nslab > 1 ? a.eps_nslab : 1;
        float e = a.eps[i];
        for (int j = 1; j < ns; ++j) e += a.eps[i + (long)j * a.eps_slab_stride];
        const float nz = a.noise[(long)st * a.noise_stride + i];
        float x0 = c[0] * x - c[1] * e;
        if (a.clip_x0) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        const float mean = c[2] * x0 + c[3] * x;
        a.x[i] = mean + c[4] * nz;
    }
    if (ONE_BLOCK && a.inc_step) {
        __syncthreads();
        if (threadIdx.x == 0) *a.step = st + 1;
    }
}

__global__ void k_keep_step_inc(int32_t* step) { *step += 1; }

extern "C" int es_ddpm_update_keep(const es_ddpm_keep_args* a, es_stream stream) {
    ES_REQUIRE(a && a->x && a->eps && a->noise && a->coef && a->step && a->x0 && a->mask && a->keep_noise && a->tab,
               "es_ddpm_update_keep: NULL argument");
    ES_REQUIRE(a->n > 0 && a->row > 0 && a->n % a->row == 0 && a->n_tab > 0 && a->coef_stride >= 5 && (long)a->keep_noise_stride >= (long)a->n &&
               (long)a->noise_stride >= (long)a->n,
               "es_ddpm_update_keep: n=%d row=%d n_tab=%d coef_stride=%d noise_stride=%d keep_noise_stride=%d (n a multiple of row, strides >= n)",
               a->n, a->row, a->n_tab, a->coef_stride, a->noise_stride, a->keep_noise_stride);
    if (a->n <= 4096) {
        hipLaunchKernelGGL(k_ddpm_update_keep<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, *a);
    } else {
        hipLaunchKernelGGL(k_ddpm_update_keep<false>, dim3((a->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
        if (a->inc_step) hipLaunchKernelGGL(k_keep_step_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, a->step);
    }
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// k_box_prescale: metric boxes -> the normalised rows of the layout state.  Column c of ncol (6: sizes | translations, 7: + a metric
// angle) becomes 2 (v - lo) / (hi - lo) - 1 with the float64 statistics of the dataset (scale_box_params, helpers/util.py:516-532, angle
// flag :528-530), and an angle becomes (sin, cos) (preprocess_angle2sincos, :534-540).  The reference computes on float64 statistics:
// everything is evaluated in double here and rounded to fp32 once -- 14 numbers per box.
// ---------------------------------------------------------------------------------------------
__global__ void k_box_prescale(const float* boxes, int ld, int ncol, const float* angles, const double* stats, float* out, int out_ld,
                               float* sincos_out, int O) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= O) return;
    if (boxes && out) {
        for (int c = 0; c < ncol; ++c) {
            const double lo = stats[c < 3 ? c : c < 6 ? 3 + c : 12], hi = stats[c < 3 ? 3 + c : c < 6 ? 6 + c : 13];
            double v = ((double)boxes[(long)i * ld + c] - lo) / (hi - lo);
            v = 2.0 * v - 1.0;
            out[(long)i * out_ld + c] = (float)v;
        }
    }
    if (angles && sincos_out) {
        const double t = (double)angles[i];
        sincos_out[2 * i] = (float)sin(t);
        sincos_out[2 * i + 1] = (float)cos(t);
    }
}

extern "C" int es_box_prescale(const float* boxes, int ld, int ncol, const float* angles, const double* stats, float* out, int out_ld,
                               float* sincos_out, int O, es_stream stream) {
    ES_REQUIRE(O > 0 && ((boxes && out) || (angles && sincos_out)), "es_box_prescale: nothing to do (O=%d)", O);
    ES_REQUIRE(!boxes == !out && !angles == !sincos_out, "es_box_prescale: boxes / out and angles / sincos_out go together");
    ES_REQUIRE(!boxes || (stats && (ncol == 6 || ncol == 7) && ld >= ncol && out_ld >= ncol),
               "es_box_prescale: bad args (ncol=%d, ld=%d, out_ld=%d)", ncol, ld, out_ld);
    hipLaunchKernelGGL(k_box_prescale, dim3((O + 63) / 64), dim3(64), 0, (hipStream_t)stream, boxes, ld, ncol, angles, stats, out, out_ld,
                       sincos_out, O);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
