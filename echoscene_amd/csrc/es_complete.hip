// Shape completion (keep PART of a given shape while the rest of it, and the other objects, are generated):
//   * k_ddim_blend_vox -- the masked-DDIM blend of DDIMSampler.ddim_sampling (samplers/ddim.py:160-163) with a mask per latent VOXEL,
//     the z_mask [B, 1, zH, zW, zD] of get_partial_shape (diffusion_shape/diff_utils/demo_util.py:229-252), as shape_comp uses it
//     (diffusion_shape/sdfusion_model.py:400-446); planned in front of every step's denoiser like k_ddim_blend (es_keep.hip);
//   * k_range_mask     -- that z_mask from integer bounds per object;
//   * k_partial_shape  -- the visualisation half of get_partial_shape (demo_util.py:207-227) on SDF grids.
#include "es_common.h"

// ---------------------------------------------------------------------------------------------
// x[o, c, v] = mask[o, v] ? tab[2 st] * x0[o, c, v] + tab[2 st + 1] * noise[st][o, c, v] : x[o, c, v]      (st = *step, not advanced)
// Two products and one sum, uncontracted: the bits of k_ddim_blend.  One lane per four consecutive voxels (16-byte accesses),
// grid.y = object; the lane reads its four mask values once and walks the C channels.  Four zeros: the lane returns before any other
// load.  Four ones: it stores without reading x.  Mixed: it reads x and selects element by element -- an element whose mask is 0 gets
// its own bits back, and what x0 / noise hold there (garbage, NaN) never enters a result.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ddim_blend_vox(const es_blend_vox_args a) {
#pragma clang fp contract(off)
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
        f4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p = ca * v0[e], q = cb * nv[e];
            r[e] = p + q;
        }
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

// ---------------------------------------------------------------------------------------------
// The reference's slice assignments (mask[:, :, :st] = 0; mask[:, :, ed:] = 0 per axis) leave 1 exactly where st <= i < ed on all
// three axes; st >= ed on any axis leaves nothing.  bounds row = (st, ed) of dim 2 ('x'), dim 3 ('y'), dim 4 ('z').
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool es_in_range(const int32_t* b, int d, int h, int w) {
    return d >= b[0] && d < b[1] && h >= b[2] && h < b[3] && w >= b[4] && w < b[5];
}

__global__ __launch_bounds__(256) void k_range_mask(const int32_t* bounds, int D, int H, int W, float* mask) {
    const int k = blockIdx.y;
    const int V = D * H * W;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int w = v % W, h = (v / W) % H, d = v / (W * H);
    mask[(long)k * V + v] = es_in_range(bounds + 6 * k, d, h, w) ? 1.0f : 0.0f;
}

extern "C" int es_range_mask(const int32_t* bounds, int K, int D, int H, int W, float* mask, es_stream stream) {
    ES_REQUIRE(bounds && mask, "es_range_mask: NULL argument");
    ES_REQUIRE(K > 0 && K <= 65535 && D > 0 && H > 0 && W > 0 && (long)D * H * W < (1L << 31),
               "es_range_mask: K=%d (1..65535), grid (%d, %d, %d)", K, D, H, W);
    const int V = D * H * W;
    hipLaunchKernelGGL(k_range_mask, dim3((V + 255) / 256, K), dim3(256), 0, (hipStream_t)stream, bounds, D, H, W, mask);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

// shape_part = inside ? sdf : fill, shape_missing = inside ? fill : sdf, shape_mask = inside (uint8); sdf [K, n, n, n]
__global__ __launch_bounds__(256) void k_partial_shape(const float* sdf, const int32_t* bounds, int n, float fill, float* part,
                                                       float* missing, uint8_t* smask) {
    const int k = blockIdx.y;
    const int V = n * n * n;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int w = v % n, h = (v / n) % n, d = v / (n * n);
    const bool in = es_in_range(bounds + 6 * k, d, h, w);
    const long i = (long)k * V + v;
    const float s = sdf[i];
    part[i] = in ? s : fill;
    missing[i] = in ? fill : s;
    smask[i] = in ? 1 : 0;
}

extern "C" int es_partial_shape(const float* sdf, const int32_t* bounds, int K, int n, float fill, float* shape_part,
                                float* shape_missing, uint8_t* shape_mask, es_stream stream) {
    ES_REQUIRE(sdf && bounds && shape_part && shape_missing && shape_mask, "es_partial_shape: NULL argument");
    ES_REQUIRE(K > 0 && K <= 65535 && n > 0 && n <= 1024, "es_partial_shape: K=%d (1..65535), n=%d (1..1024)", K, n);
    const int V = n * n * n;
    hipLaunchKernelGGL(k_partial_shape, dim3((V + 255) / 256, K), dim3(256), 0, (hipStream_t)stream, sdf, bounds, n, fill, shape_part,
                       shape_missing, shape_mask);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
