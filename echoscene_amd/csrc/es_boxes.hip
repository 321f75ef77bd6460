// Layout boxes between metric and normalised form (helpers/util.py:516-568):
//   * k_box_prescale    -- scale_box_params + preprocess_angle2sincos (:516-540): metric boxes -> the normalised rows of the layout
//     state, so that a given box can be kept while sampling; evaluated in double;
//   * k_box_postprocess -- descale_box_params + postprocess_sincos2arctan (:542-568), its inverse after the layout loop; fp32.
#include "es_common.h"

namespace {

// stats = {min_lhw[3], max_lhw[3], min_xyz[3], max_xyz[3], min_angle, max_angle}: the range of column c of sizes | translations | angle
template <class T>
__device__ __forceinline__ void box_range(const T* stats, int c, T& lo, T& hi) {
    lo = stats[c < 3 ? c : c < 6 ? 3 + c : 12];
    hi = stats[c < 3 ? 3 + c : c < 6 ? 6 + c : 13];
}

// ---------------------------------------------------------------------------------------------
// k_box_prescale: column c of ncol (6: sizes | translations, 7: + a metric angle) becomes 2 (v - lo) / (hi - lo) - 1 with the float64
// statistics of the dataset (scale_box_params, helpers/util.py:516-532, angle flag :528-530), and an angle becomes (sin, cos)
// (preprocess_angle2sincos, :534-540).  The reference computes on float64 statistics: everything is evaluated in double here and
// rounded to fp32 once -- 14 numbers per box.
// ---------------------------------------------------------------------------------------------
__global__ void k_box_prescale(const float* boxes, int ld, int ncol, const float* angles, const double* stats, float* out, int out_ld,
                               float* sincos_out, int O) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= O) return;
    if (boxes && out) {
        for (int c = 0; c < ncol; ++c) {
            double lo, hi;
            box_range(stats, c, lo, hi);
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

// Box de-normalisation after the layout loop (helpers/util.py:542-568): [-1,1] -> [min,max] for sizes and translations (in place)
// and (sin, cos) -> arctan2 in degrees-or-radians (scale).
// ncol = 7: also the angle column (descale_box_params(angle=True), helpers/util.py:553-555: stats[12], stats[13]).
__global__ void k_box_postprocess(float* boxes, int ld, const float* sincos, float* angle_out, const float* stats,
                                  int O, float angle_scale, int ncol) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= O) return;
    if (boxes) {
        for (int c = 0; c < ncol; ++c) {
            float lo, hi;
            box_range(stats, c, lo, hi);
            float v = boxes[(long)i * ld + c];
            v = (v + 1.0f) / 2.0f;
            boxes[(long)i * ld + c] = v * (hi - lo) + lo;
        }
    }
    if (sincos && angle_out) angle_out[i] = atan2f(sincos[2 * i], sincos[2 * i + 1]) * angle_scale;
}

}  // namespace

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

extern "C" int es_box_postprocess(float* boxes, int ld, const float* sincos, float* angle_out, const float* stats,
                                  int O, float angle_scale, es_stream stream) {
    ES_REQUIRE(O > 0 && (!boxes || (stats && ld >= 6)), "es_box_postprocess: bad args");
    hipLaunchKernelGGL(k_box_postprocess, dim3((O + 63) / 64), dim3(64), 0, (hipStream_t)stream, boxes, ld, sincos,
                       angle_out, stats, O, angle_scale, 6);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_box_descale(float* boxes, int ld, int ncol, const float* stats, int O, es_stream stream) {
    ES_REQUIRE(O > 0 && boxes && stats && (ncol == 6 || ncol == 7) && ld >= ncol, "es_box_descale: bad args (ncol=%d, ld=%d)", ncol, ld);
    hipLaunchKernelGGL(k_box_postprocess, dim3((O + 63) / 64), dim3(64), 0, (hipStream_t)stream, boxes, ld, (const float*)nullptr,
                       (float*)nullptr, stats, O, 1.0f, ncol);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
