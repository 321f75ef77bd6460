// Every sampler state update, and each step's arithmetic written once:
//   * k_update_rows    -- the layout loop's update as ONE launch of its latency-bound step: ancestral DDPM (p_sample_sg, diffusion_ddpm.py:
//     296-309) or strided DDIM (DDIMSampler.p_sample_ddim, samplers/ddim.py:236-262), with or without kept rows (keep given boxes
//     while the others are placed around them); es_ddpm_update, es_ddpm_update_keep and es_ddim_rows_update launch it;
//   * k_ddim_update    -- the shape loop's per-step DDIM update (es_ddim_update);
//   * k_plms           -- PLMS sampling of the shape branch (PLMSSampler.p_sample_plms, samplers/plms.py:179-247): pseudo linear multistep
//     on the DDIM schedule;
//   * k_ddim_blend, k_ddim_blend_vox -- the masked-DDIM blend of DDIMSampler.ddim_sampling (samplers/ddim.py:160-163) with q_sample
//     (echo2shape.py:254-258), planned in front of every step's denoiser: a mask per object (keep given shapes) or per latent VOXEL, the
//     z_mask [B, 1, zH, zW, zD] of get_partial_shape (diff_utils/demo_util.py:229-252) as shape_comp uses it (sdfusion_model.py:400-446).
// Every expression is the reference's, in its order: scalar * tensor products, sums left to right, true divisions, and no fused
// multiply-add anywhere in this file (the pragma below).  The masked loops equal the unmasked ones on the free rows, and a kept row's
// q_sample equals the blend's, bit for bit, because both sides call the same helper.

#pragma clang fp contract(off)

#include "es_common.h"

namespace {

// The deferred split-K reduction of the denoiser's last product: slab 0, + slab 1, ... in that fixed order (nslab >= 1; the argument
// structs say 0 or 1 for a plain tensor).
__device__ __forceinline__ float slab_sum(const float* p, int nslab, long slab_stride) {
    float v = *p;
    for (int j = 1; j < nslab; ++j) v += p[(long)j * slab_stride];
    return v;
}
__device__ __forceinline__ f4 slab_sum4(const float* p, int nslab, long slab_stride) {
    f4 v = *(const f4*)p;
    for (int j = 1; j < nslab; ++j) v += *(const f4*)(p + (long)j * slab_stride);
    return v;
}

// p_mean_variance + p_sample_sg (diffusion_ddpm.py:220-264, 296-309); clip: clip_denoised=True, torch.clamp(x_recon, -1, 1) (:243-244)
__device__ __forceinline__ float ddpm_step(float x, float e, float nz, const float* c, bool clip) {
    float x0 = c[0] * x - c[1] * e;
    if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    const float mean = c[2] * x0 + c[3] * x;
    return mean + c[4] * nz;
}

// p_sample_ddim (samplers/ddim.py:236-262), get_x_prev_and_pred_x0 (plms.py:206-227) at sigma_t = 0
__device__ __forceinline__ float ddim_step(float x, float e, const float* c) {
    const float px0 = (x - c[0] * e) / c[1];
    return c[2] * px0 + c[3] * e;
}
__device__ __forceinline__ f4 ddim_step4(const f4 x, const f4 e, const float* c) {
    f4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = ddim_step(x[k], e[k], c);
    return r;
}
// eta != 0 (samplers/ddim.py:256-260): + sigma_t * randn; c[3] then already is sqrt(1 - a_prev - sigma_t^2), c[4] = sigma_t.
// noise = NULL: eta = 0
__device__ __forceinline__ float ddim_step_eta(float x, float e, const float* c, const float* noise, long at) {
    float xn = ddim_step(x, e, c);
    if (noise) xn = xn + c[4] * noise[at];
    return xn;
}

// q_sample (GaussianDiffusion.q_sample, diffusion_ddpm.py:191-201; echo2shape.py:254-258): two products and a sum.  The reference
// blends with a 0 / 1 mask -- img_orig * 1 + 0 * img is img_orig, img_orig * 0 + 1 * img is img -- so a kept element is these bits.
__device__ __forceinline__ float q_sample(float ca, float v, float cb, float nz) {
    const float p = ca * v, q = cb * nz;
    return p + q;
}
__device__ __forceinline__ f4 q_sample4(float ca, const f4 v, float cb, const f4 nz) {
    f4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = q_sample(ca, v[k], cb, nz[k]);
    return r;
}

__global__ void k_step_inc(int32_t* step) { *step += 1; }
__global__ void k_step_set(int32_t* step, int32_t v) { *step = v; }

// ---------------------------------------------------------------------------------------------
// k_update_rows: one update of the layout state x [n / row, row].  A row whose mask is 0 -- every row when mask is NULL, and then
// nothing of x0 / tab / keep_noise / row is read -- takes the DDPM or the DDIM step.  A row whose mask is 1 gets the state the denoiser
// of the NEXT iteration has to see:
//     st + 1 <  n_tab:  x[i] = q_sample of x0[i] with tab[st+1] and keep_noise[st+1][i]
//     st + 1 == n_tab:  x[i] = x0[i]                                                                (the loop's result: the caller's bits)
// A kept element reads neither eps nor the step's noise draw, and is never clipped; row st + 1 of tab / keep_noise is only touched
// when it exists.  ONE_BLOCK: the whole state in one workgroup (n <= 4096: one scene) -- the step counter is advanced by the same
// kernel, after every thread has read it (a launch less per step of the latency-bound layout loop).
// ---------------------------------------------------------------------------------------------
template <bool DDIM, bool ONE_BLOCK>
__global__ void k_update_rows(const es_ddpm_keep_args a) {
    const int st = *a.step;
    const float* c = a.coef + (long)st * a.coef_stride;
    const bool last = st + 1 >= a.n_tab;
    float ka = 0.0f, kb = 0.0f;
    if (a.mask && !last) { ka = a.tab[2 * (st + 1)]; kb = a.tab[2 * (st + 1) + 1]; }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += ONE_BLOCK ? (int)blockDim.x : a.n) {
        if (a.mask && a.mask[i / a.row] != 0.0f) {
            float v = a.x0[i];
            if (!last) v = q_sample(ka, v, kb, a.keep_noise[(long)(st + 1) * a.keep_noise_stride + i]);
            a.x[i] = v;
            continue;
        }
        const float x = a.x[i], e = slab_sum(a.eps + i, a.eps_nslab > 1 ? a.eps_nslab : 1, a.eps_slab_stride);
        const long at = (long)st * a.noise_stride + i;
        a.x[i] = DDIM ? ddim_step_eta(x, e, c, a.noise, at) : ddpm_step(x, e, a.noise[at], c, a.clip_x0);
    }
    if (ONE_BLOCK && a.inc_step) {
        __syncthreads();
        if (threadIdx.x == 0) *a.step = st + 1;
    }
}

template <bool DDIM>
int update_rows(const es_ddpm_keep_args& a, es_stream stream) {
    if (a.n <= 4096) {
        hipLaunchKernelGGL((k_update_rows<DDIM, true>), dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL((k_update_rows<DDIM, false>), dim3((a.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
        if (a.inc_step) hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, a.step);
    }
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ void k_ddim_update(const es_update_args a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int st = *a.step;
    if (i < a.n) {
        const float* c = a.coef + (long)st * a.coef_stride;
        const float x = a.x[i], e = slab_sum(a.eps + i, a.eps_nslab > 1 ? a.eps_nslab : 1, a.eps_slab_stride);
        a.x[i] = ddim_step_eta(x, e, c, a.noise, (long)st * a.noise_stride + i);
    }
}

// ---------------------------------------------------------------------------------------------
// k_plms.  The sampler's state next to the latents x is a ring of the last three eps [3][ring_stride] (fp32) and, for the
// improved-Euler first iteration, a copy of x.  Three launches, one kernel template:
//   * UPDATE  -- the steady iteration st = *step >= 1 (Adams-Bashforth of order min(st, 3) + 1 on eps and the ring), st advanced after;
//   * FIRST_A -- iteration 0 after the first evaluation: xsave = x, ring[0] = e, x = DDIM step of x with e, *step = 1;
//   * FIRST_B -- iteration 0 after the second evaluation (of x at time-embedding row 1): x = DDIM step of xsave with (ring[0] + e) / 2.
// One lane per 16 bytes; no lane reads what another writes.
// ---------------------------------------------------------------------------------------------
enum { PLMS_UPDATE = 0, PLMS_FIRST_A = 1, PLMS_FIRST_B = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void k_plms(const es_plms_args a) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= a.n) return;
    const f4 e = slab_sum4(a.eps + i, a.eps_nslab > 1 ? a.eps_nslab : 1, a.eps_slab_stride);
    if (MODE == PLMS_FIRST_A) {
        const f4 x = *(const f4*)(a.x + i);
        *(f4*)(a.xsave + i) = x;
        *(f4*)(a.ring + i) = e;
        *(f4*)(a.x + i) = ddim_step4(x, e, a.coef);
        return;
    }
    if (MODE == PLMS_FIRST_B) {
        const f4 h = *(const f4*)(a.ring + i);
        f4 ep;
#pragma unroll
        for (int k = 0; k < 4; ++k) ep[k] = (h[k] + e[k]) / 2.0f;
        *(f4*)(a.x + i) = ddim_step4(*(const f4*)(a.xsave + i), ep, a.coef);
        return;
    }
    const int st = *a.step;                                   // >= 1 (es_plms_first_a left 1): wave-uniform, so is the order branch
    const float* c = a.coef + (long)st * a.coef_stride;
    float* const slot = a.ring + (long)(st % 3) * a.ring_stride + i;             // this iteration's slot: it holds h3
    const f4 h1 = *(const f4*)(a.ring + (long)((st + 2) % 3) * a.ring_stride + i);
    f4 ep;
    if (st <= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ep[k] = (3.0f * e[k] - h1[k]) / 2.0f;
    } else {
        const f4 h2 = *(const f4*)(a.ring + (long)((st + 1) % 3) * a.ring_stride + i);
        if (st == 2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ep[k] = (23.0f * e[k] - 16.0f * h1[k] + 5.0f * h2[k]) / 12.0f;
        } else {
            const f4 h3 = *(const f4*)slot;                   // read before the slot is overwritten below
#pragma unroll
            for (int k = 0; k < 4; ++k) ep[k] = (55.0f * e[k] - 59.0f * h1[k] + 37.0f * h2[k] - 9.0f * h3[k]) / 24.0f;
        }
    }
    const f4 x = *(const f4*)(a.x + i);
    *(f4*)slot = e;                                           // the history keeps e, not e' (plms.py:166-167, 247)
    *(f4*)(a.x + i) = ddim_step4(x, ep, c);
}

int plms_check(const es_plms_args* a, const char* who, bool first) {
    ES_REQUIRE(a && a->x && a->eps && a->coef && a->step && a->ring && (!first || a->xsave), "%s: NULL argument", who);
    ES_REQUIRE(a->n > 0 && a->n % 4 == 0 && a->coef_stride >= 4 && a->ring_stride >= a->n && a->ring_stride % 4 == 0,
               "%s: n=%d coef_stride=%d ring_stride=%d (n and the ring stride multiples of 4, ring stride >= n, coef stride >= 4)", who, a->n,
               a->coef_stride, a->ring_stride);
    ES_REQUIRE(a->eps_nslab <= 1 || (a->eps_slab_stride > 0 && a->eps_slab_stride % 4 == 0), "%s: eps_nslab=%d eps_slab_stride=%d (a multiple of 4)",
               who, a->eps_nslab, a->eps_slab_stride);
    ES_REQUIRE((((uintptr_t)a->x | (uintptr_t)a->eps | (uintptr_t)a->ring | (uintptr_t)a->xsave) & 15) == 0,
               "%s: x, eps, ring and xsave must be 16-byte aligned", who);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// x[o, :] = mask[o] ? q_sample of x0[o, :] with tab[st] and noise[st][o, :] : x[o, :]          (st = *step, not advanced)
// A kept row is the q_sample bits and any other row is left alone (neither read nor written).  One lane per 16 bytes, grid.y = object.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ddim_blend(const es_blend_args a) {
    const int o = blockIdx.y;
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= a.n || a.mask[o] == 0.0f) return;
    const int st = *a.step;
    const float ca = a.tab[2 * st], cb = a.tab[2 * st + 1];
    const long row = (long)o * a.n + i;
    const f4 v0 = *(const f4*)(a.x0 + row);
    const f4 nz = *(const f4*)(a.noise + (long)st * a.noise_stride + row);
    *(f4*)(a.x + row) = q_sample4(ca, v0, cb, nz);
}

// ---------------------------------------------------------------------------------------------
// x[o, c, v] = mask[o, v] ? q_sample of x0[o, c, v] with tab[st] and noise[st][o, c, v] : x[o, c, v]      (st = *step, not advanced)
// One lane per four consecutive voxels (16-byte accesses), grid.y = object; the lane reads its four mask values once and walks the C
// channels.  Four zeros: the lane returns before any other load.  Four ones: it stores without reading x.  Mixed: it reads x and
// selects element by element -- an element whose mask is 0 gets its own bits back, and what x0 / noise hold there (garbage, NaN)
// never enters a result.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ddim_blend_vox(const es_blend_vox_args a) {
    const int o = blockIdx.y;
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= a.V) return;
    const f4 m = *(const f4*)(a.mask + (long)o * a.V + i);
    const bool k0 = m[0] != 0.0f, k1 = m[1] != 0.0f, k2 = m[2] != 0.0f, k3 = m[3] != 0.0f;
    if (!(k0 || k1 || k2 || k3)) return;
    const bool all = k0 && k1 && k2 && k3;
    const int st = *a.step;
    const float ca = a.tab[2 * st], cb = a.tab[2 * st + 1];
    const float* nz = a.noise + (long)st * a.noise_stride;
    for (int c = 0; c < a.C; ++c) {
        const long row = ((long)o * a.C + c) * a.V + i;
        const f4 v0 = *(const f4*)(a.x0 + row);
        const f4 nv = *(const f4*)(nz + row);
        f4 r = q_sample4(ca, v0, cb, nv);
        if (!all) {
            const f4 xv = *(const f4*)(a.x + row);
            r[0] = k0 ? r[0] : xv[0];
            r[1] = k1 ? r[1] : xv[1];
            r[2] = k2 ? r[2] : xv[2];
            r[3] = k3 ? r[3] : xv[3];
        }
        *(f4*)(a.x + row) = r;
    }
}

}  // namespace

// es_update_args is the first twelve members of es_ddpm_keep_args; the rest stays zero: no mask, and nothing behind it is read
extern "C" int es_ddpm_update(const es_update_args* a, es_stream stream) {
    ES_REQUIRE(a->n > 0 && a->step && a->noise, "es_ddpm_update: bad args");
    es_ddpm_keep_args k = {};
    k.x = a->x; k.eps = a->eps; k.eps_nslab = a->eps_nslab; k.eps_slab_stride = a->eps_slab_stride;
    k.noise = a->noise; k.noise_stride = a->noise_stride; k.coef = a->coef; k.coef_stride = a->coef_stride;
    k.step = a->step; k.n = a->n; k.inc_step = a->inc_step; k.clip_x0 = a->clip_x0;
    return update_rows<false>(k, stream);
}

extern "C" int es_ddpm_update_keep(const es_ddpm_keep_args* a, es_stream stream) {
    ES_REQUIRE(a && a->x && a->eps && a->noise && a->coef && a->step && a->x0 && a->mask && a->keep_noise && a->tab,
               "es_ddpm_update_keep: NULL argument");
    ES_REQUIRE(a->n > 0 && a->row > 0 && a->n % a->row == 0 && a->n_tab > 0 && a->coef_stride >= 5 && (long)a->keep_noise_stride >= (long)a->n &&
               (long)a->noise_stride >= (long)a->n,
               "es_ddpm_update_keep: n=%d row=%d n_tab=%d coef_stride=%d noise_stride=%d keep_noise_stride=%d (n a multiple of row, strides >= n)",
               a->n, a->row, a->n_tab, a->coef_stride, a->noise_stride, a->keep_noise_stride);
    return update_rows<false>(*a, stream);
}

extern "C" int es_ddim_rows_update(const es_ddpm_keep_args* a, es_stream stream) {
    ES_REQUIRE(a && a->x && a->eps && a->coef && a->step, "es_ddim_rows_update: NULL argument");
    ES_REQUIRE(!a->mask == !a->x0 && !a->mask == !a->keep_noise && !a->mask == !a->tab,
               "es_ddim_rows_update: mask, x0, keep_noise and tab go together (all given or all NULL)");
    ES_REQUIRE(a->clip_x0 == 0, "es_ddim_rows_update: clip_x0 is not defined for DDIM (the reference's p_sample_ddim never clips)");
    ES_REQUIRE(a->n > 0 && a->row > 0 && a->n % a->row == 0 && a->n_tab > 0 && a->coef_stride >= (a->noise ? 5 : 4) &&
               (!a->noise || (long)a->noise_stride >= (long)a->n) && (!a->mask || (long)a->keep_noise_stride >= (long)a->n) &&
               (a->eps_nslab <= 1 || (long)a->eps_slab_stride >= (long)a->n),
               "es_ddim_rows_update: n=%d row=%d n_tab=%d coef_stride=%d noise_stride=%d keep_noise_stride=%d eps_nslab=%d eps_slab_stride=%d "
               "(n a multiple of row, strides >= n, coef stride >= 4, 5 with noise)",
               a->n, a->row, a->n_tab, a->coef_stride, a->noise_stride, a->keep_noise_stride, a->eps_nslab, a->eps_slab_stride);
    return update_rows<true>(*a, stream);
}

extern "C" int es_ddim_update(const es_update_args* a, es_stream stream) {
    ES_REQUIRE(a->n > 0 && a->step, "es_ddim_update: bad args");
    hipLaunchKernelGGL(k_ddim_update, dim3((a->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    if (a->inc_step) hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, a->step);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_plms_update(const es_plms_args* a, es_stream stream) {
    if (int rc = plms_check(a, "es_plms_update", false)) return rc;
    hipLaunchKernelGGL(k_plms<PLMS_UPDATE>, dim3((a->n / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    if (a->inc_step) hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, a->step);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_plms_first_a(const es_plms_args* a, es_stream stream) {
    if (int rc = plms_check(a, "es_plms_first_a", true)) return rc;
    hipLaunchKernelGGL(k_plms<PLMS_FIRST_A>, dim3((a->n / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    hipLaunchKernelGGL(k_step_set, dim3(1), dim3(1), 0, (hipStream_t)stream, a->step, 1);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_plms_first_b(const es_plms_args* a, es_stream stream) {
    if (int rc = plms_check(a, "es_plms_first_b", true)) return rc;
    hipLaunchKernelGGL(k_plms<PLMS_FIRST_B>, dim3((a->n / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
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

extern "C" int es_ddim_blend_vox(const es_blend_vox_args* a, es_stream stream) {
    ES_REQUIRE(a && a->x && a->x0 && a->mask && a->noise && a->tab && a->step, "es_ddim_blend_vox: NULL argument");
    ES_REQUIRE(a->O > 0 && a->C > 0 && a->V > 0 && a->V % 4 == 0 && a->noise_stride % 4 == 0 &&
               (long)a->noise_stride >= (long)a->O * a->C * a->V,
               "es_ddim_blend_vox: O=%d C=%d V=%d noise_stride=%d (V and the stride multiples of 4, stride >= O * C * V)", a->O, a->C, a->V,
               a->noise_stride);
    ES_REQUIRE(a->O <= 65535, "es_ddim_blend_vox: O=%d objects (<= 65535)", a->O);
    ES_REQUIRE((((uintptr_t)a->x | (uintptr_t)a->x0 | (uintptr_t)a->mask | (uintptr_t)a->noise) & 15) == 0,
               "es_ddim_blend_vox: x, x0, mask and noise must be 16-byte aligned");
    hipLaunchKernelGGL(k_ddim_blend_vox, dim3((a->V / 4 + 255) / 256, a->O), dim3(256), 0, (hipStream_t)stream, *a);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
