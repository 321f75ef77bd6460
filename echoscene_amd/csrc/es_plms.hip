// PLMS sampling of the shape branch (PLMSSampler.p_sample_plms, diffusion_shape/samplers/plms.py:179-247): pseudo linear multistep on
// the DDIM schedule.  The sampler's state next to the latents x is a ring of the last three eps [3][ring_stride] (fp32) and, for the
// improved-Euler first iteration, a copy of x.  Three launches, one kernel template:
//   * UPDATE  -- the steady iteration st = *step >= 1 (Adams-Bashforth of order min(st, 3) + 1 on eps and the ring), st advanced after;
//   * FIRST_A -- iteration 0 after the first evaluation: xsave = x, ring[0] = e, x = DDIM step of x with e, *step = 1;
//   * FIRST_B -- iteration 0 after the second evaluation (of x at time-embedding row 1): x = DDIM step of xsave with (ring[0] + e) / 2.
// Every expression is the reference's, in its order, uncontracted: scalar * tensor products, sums left to right, one true division.
// One lane per 16 bytes; no lane reads what another writes.
#include "es_common.h"

enum { PLMS_UPDATE = 0, PLMS_FIRST_A = 1, PLMS_FIRST_B = 2 };

// get_x_prev_and_pred_x0 (plms.py:206-227) at sigma_t = 0 -- k_ddim_update's two lines
__device__ __forceinline__ f4 plms_ddim_step(const f4 x, const f4 e, const float* c) {
#pragma clang fp contract(off)
    f4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float px0 = (x[k] - c[0] * e[k]) / c[1];
        r[k] = c[2] * px0 + c[3] * e[k];
    }
    return r;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_plms(const es_plms_args a) {
#pragma clang fp contract(off)
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= a.n) return;
    // the fixed-order slab sum of eps (k_ddim_update: slab 0, + slab 1, ...)
    const int ns = a.eps_nslab > 1 ? a.eps_nslab : 1;
    f4 e = *(const f4*)(a.eps + i);
    for (int j = 1; j < ns; ++j) e += *(const f4*)(a.eps + (long)j * a.eps_slab_stride + i);
    if (MODE == PLMS_FIRST_A) {
        const f4 x = *(const f4*)(a.x + i);
        *(f4*)(a.xsave + i) = x;
        *(f4*)(a.ring + i) = e;
        *(f4*)(a.x + i) = plms_ddim_step(x, e, a.coef);
        return;
    }
    if (MODE == PLMS_FIRST_B) {
        const f4 h = *(const f4*)(a.ring + i);
        f4 ep;
#pragma unroll
        for (int k = 0; k < 4; ++k) ep[k] = (h[k] + e[k]) / 2.0f;
        *(f4*)(a.x + i) = plms_ddim_step(*(const f4*)(a.xsave + i), ep, a.coef);
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
    *(f4*)(a.x + i) = plms_ddim_step(x, ep, c);
}

__global__ void k_plms_step_inc(int32_t* step) { *step += 1; }
__global__ void k_plms_step_set(int32_t* step, int32_t v) { *step = v; }

static int plms_check(const es_plms_args* a, const char* who, bool first) {
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

extern "C" int es_plms_update(const es_plms_args* a, es_stream stream) {
    if (int rc = plms_check(a, "es_plms_update", false)) return rc;
    hipLaunchKernelGGL(k_plms<PLMS_UPDATE>, dim3((a->n / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    if (a->inc_step) hipLaunchKernelGGL(k_plms_step_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, a->step);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_plms_first_a(const es_plms_args* a, es_stream stream) {
    if (int rc = plms_check(a, "es_plms_first_a", true)) return rc;
    hipLaunchKernelGGL(k_plms<PLMS_FIRST_A>, dim3((a->n / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    hipLaunchKernelGGL(k_plms_step_set, dim3(1), dim3(1), 0, (hipStream_t)stream, a->step, 1);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_plms_first_b(const es_plms_args* a, es_stream stream) {
    if (int rc = plms_check(a, "es_plms_first_b", true)) return rc;
    hipLaunchKernelGGL(k_plms<PLMS_FIRST_B>, dim3((a->n / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
