// Shape completion (keep PART of a given shape while the rest of it, and the other objects, are generated): the masks and the
// visualisation around the voxel blend k_ddim_blend_vox (es_update.hip):
//   * k_range_mask     -- the z_mask [B, 1, zH, zW, zD] of get_partial_shape (diffusion_shape/diff_utils/demo_util.py:229-252) from
//     integer bounds per object;
//   * k_partial_shape  -- the visualisation half of get_partial_shape (demo_util.py:207-227) on SDF grids.
#include "es_common.h"

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
