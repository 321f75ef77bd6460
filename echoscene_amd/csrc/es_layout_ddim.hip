// Strided DDIM sampling of the layout branch (DDIMSampler.p_sample_ddim, diffusion_shape/samplers/ddim.py:236-262, driven on the layout
// denoiser): the update of a loop on rows [O, row], as ONE launch of the latency-bound layout step.
//   * k_ddim_rows_update -- on the rows whose mask is 0 (or with no mask at all) es_ddim_update's arithmetic, the same expressions in
//     the same order as k_ddim_update (es_rows.hip): the same bits; on the rows whose mask is 1 what k_ddpm_update_keep (es_keep.hip)
//     leaves there -- the NEXT iteration's q_sample of x0, or x0 itself after the last iteration.
// es_ddim_update is two launches when it advances the step counter and has no masked form; ONE_BLOCK (n <= 4096: one scene) keeps the
// whole state in one workgroup, which advances the counter itself after every thread has read it.
#include "es_common.h"

template <bool ONE_BLOCK>
__global__ void k_ddim_rows_update(const es_ddpm_keep_args a) {
#pragma clang fp contract(off)
    const int st = *a.step;
    const float* c = a.coef + (long)st * a.coef_stride;
    const bool last = st + 1 >= a.n_tab;
    float ka = 0.0f, kb = 0.0f;
    if (a.mask && !last) { ka = a.tab[2 * (st + 1)]; kb = a.tab[2 * (st + 1) + 1]; }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += ONE_BLOCK ? (int)blockDim.x : a.n) {
        if (a.mask && a.mask[i / a.row] != 0.0f) {
            float v = a.x0[i];
            if (!last) {
                const float p = ka * v, q = kb * a.keep_noise[(long)(st + 1) * a.keep_noise_stride + i];
                v = p + q;
            }
            a.x[i] = v;
            continue;
        }
        const float x = a.x[i];
        // the fixed-order slab sum of eps (k_ddim_update: slab 0, + slab 1, ...)
        const int ns = a.eps_nslab > 1 ? a.eps_nslab : 1;
        float e = a.eps[i];
        for (int j = 1; j < ns; ++j) e += a.eps[i + (long)j * a.eps_slab_stride];
        const float px0 = (x - c[0] * e) / c[1];
        float xn = c[2] * px0 + c[3] * e;
        // eta != 0: + sigma_t * randn; c[3] then already is sqrt(1 - a_prev - sigma_t^2), c[4] = sigma_t
        if (a.noise) xn = xn + c[4] * a.noise[(long)st * a.noise_stride + i];
        a.x[i] = xn;
    }
    if (ONE_BLOCK && a.inc_step) {
        __syncthreads();
        if (threadIdx.x == 0) *a.step = st + 1;
    }
}

__global__ void k_ddim_rows_step_inc(int32_t* step) { *step += 1; }

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
    if (a->n <= 4096) {
        hipLaunchKernelGGL(k_ddim_rows_update<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, *a);
    } else {
        hipLaunchKernelGGL(k_ddim_rows_update<false>, dim3((a->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
        if (a->inc_step) hipLaunchKernelGGL(k_ddim_rows_step_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, a->step);
    }
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
