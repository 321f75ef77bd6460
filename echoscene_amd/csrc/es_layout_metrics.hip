// Layout metrics: the scene-graph constraint accuracy of the reference's helpers/metrics_3dfront.py (validate_constrains,
// validate_constrains_changes, box3d_iou), the row L/R, F/B, Bi/Sm, Ta/Sh, Stand, Close, Symm, Total that its scripts/eval_3dfront.py
// prints.  The reference walks the triples in Python and fetches both boxes of every triple from the device; here a whole test set
// (scenes concatenated with node offsets) is one launch.
//
//   k_relation_check : one thread per triple (s, p, o).  rule_of_pred[p] names the rule (LM_LEFT .. LM_SYMM, -1: the predicate has none);
//                      the thread reads its two box rows, evaluates the rule and writes rule[t] and ok[t].  Counts per rule (ok,
//                      evaluated) are integer atomics, LDS first, then one global add per rule and workgroup: integers, so the totals do
//                      not depend on the order of arrival.
//   k_box3d_iou      : one thread per pair of boxes.
//
// Arithmetic: the reference's, operation by operation, as numpy 2 evaluates it on float32 boxes.
//   fp32 : centre differences, volume and height quotients, |dy| of standing on, the flipped-centre distances of symmetrical to; every
//          operation rounded on its own (no contraction: the pragma below, plain operators), correctly rounded quotient and root,
//          thresholds rounded to float32, the reference's strict inequalities, NaN compares false.
//   fp64 : the corners (+-l/2 + tz, +-w/2 + tx with the halves formed in fp32, h + ty), box3d_iou, the corner distances of close by.
// box3d_iou never rotates: the footprints are the rectangles (z, x) of corners 0..3; box 1 is clipped against box 2 by
// Sutherland-Hodgman with the strict `inside` test (touching boxes: nothing; a box 2 with l * w <= 0: nothing), the area of the result by
// the shoelace formula where the reference builds a convex hull (which raises on a flat result; here that is area 0).
// close by: the reference expands |a|^2 + |b|^2 - 2 a.b; the differences are taken directly here, which agrees to about 1e-14 at scene
// scale and, like the reference, counts a NaN distance as close (NaN > 0.45 is false).
//
// Indices: a node index outside [0, O) or a predicate outside [0, n_pred) raises a bit of the status word, the triple gets rule -1,
// and nothing is read through the index.

// No multiply is fused with an add in this unit.  The arithmetic below uses plain operators, not the __f*_rn helpers of the HIP
// headers: those are plain operators too, compiled under the headers' own default (contract), and fuse once they are inlined.
#pragma clang fp contract(off)

#include "es_common.h"

namespace {

constexpr int LM_BLOCK = 256;
constexpr int LM_RULES = 11;
enum { LM_LEFT = 0, LM_RIGHT, LM_FRONT, LM_BEHIND, LM_SMALLER, LM_BIGGER, LM_SHORTER, LM_TALLER, LM_STAND, LM_CLOSE, LM_SYMM };
constexpr int LM_POLY = 16;                    // room for a clipped polygon (a rectangle clipped by four lines has at most 8 vertices)

struct lm_box { float l, h, w, px, py, pz; };  // l along z, h along y, w along x; (px, py, pz) the bottom centre

__device__ __forceinline__ lm_box lm_load(const float* row) { return lm_box{row[0], row[1], row[2], row[3], row[4], row[5]}; }

// corners_from_box: z and x of corners 0..3 (corners 4..7 repeat them), the top and the bottom
struct lm_corners { double z[4], x[4], top, bottom; };

__device__ __forceinline__ lm_corners lm_corners_of(const lm_box& b, bool with_translation) {
    const float hl = (b.l / 2.0f), hw = (b.w / 2.0f);
    const double tx = with_translation ? (double)b.px : 0.0, ty = with_translation ? (double)b.py : 0.0,
                 tz = with_translation ? (double)b.pz : 0.0;
    lm_corners c;
    c.x[0] = (double)hw + tx;  c.x[1] = (double)hw + tx;  c.x[2] = (double)-hw + tx;  c.x[3] = (double)-hw + tx;
    c.z[0] = (double)hl + tz;  c.z[1] = (double)-hl + tz; c.z[2] = (double)-hl + tz;  c.z[3] = (double)hl + tz;
    c.top = (double)b.h + ty;
    c.bottom = 0.0 + ty;
    return c;
}

// poly_area of the footprint: 0.5 |sum u_i v_(i-1) - sum v_i u_(i-1)|, u = z, v = x
__device__ __forceinline__ double lm_rect_area(const lm_corners& c) {
    double p = 0.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 3) & 3;
        p += c.z[i] * c.x[j];
        q += c.x[i] * c.z[j];
    }
    return 0.5 * fabs(p - q);
}

// box3d_vol: the three edge lengths as corner distances, multiplied left to right
__device__ __forceinline__ double lm_vol(const lm_corners& c) {
    const double dz = c.z[0] - c.z[1], dx = c.x[1] - c.x[2], dy = c.top - c.bottom;
    return sqrt(dz * dz) * sqrt(dx * dx) * sqrt(dy * dy);
}

// polygon_clip(rect1, rect2) and the area of what is left
__device__ double lm_clip_area(const lm_corners& c1, const lm_corners& c2) {
    double ax[LM_POLY], ay[LM_POLY], bx[LM_POLY], by[LM_POLY];      // the list being read and the list being written, as (z, x)
    int na = 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) { ax[i] = c1.z[i]; ay[i] = c1.x[i]; }
    double cp1x = c2.z[3], cp1y = c2.x[3];
    for (int k = 0; k < 4; ++k) {
        const double cp2x = c2.z[k], cp2y = c2.x[k];
        const double ex = cp2x - cp1x, ey = cp2y - cp1y;
        int nb = 0;
        double sx = ax[na - 1], sy = ay[na - 1];
        bool s_in = ex * (sy - cp1y) > ey * (sx - cp1x);
        for (int i = 0; i < na; ++i) {
            const double px = ax[i], py = ay[i];
            const bool e_in = ex * (py - cp1y) > ey * (px - cp1x);
            if (e_in != s_in) {                                     // the edge s -> e crosses the clip line
                const double dc0 = cp1x - cp2x, dc1 = cp1y - cp2y, dp0 = sx - px, dp1 = sy - py;
                const double n1 = cp1x * cp2y - cp1y * cp2x, n2 = sx * py - sy * px;
                const double n3 = 1.0 / (dc0 * dp1 - dc1 * dp0);
                if (nb < LM_POLY) { bx[nb] = (n1 * dp0 - n2 * dc0) * n3; by[nb] = (n1 * dp1 - n2 * dc1) * n3; ++nb; }
            }
            if (e_in && nb < LM_POLY) { bx[nb] = px; by[nb] = py; ++nb; }
            sx = px; sy = py; s_in = e_in;
        }
        if (nb == 0) return 0.0;
        for (int i = 0; i < nb; ++i) { ax[i] = bx[i]; ay[i] = by[i]; }
        na = nb;
        cp1x = cp2x; cp1y = cp2y;
    }
    double p = 0.0, q = 0.0;
    for (int i = 0; i < na; ++i) {
        const int j = i == 0 ? na - 1 : i - 1;
        p += ax[i] * ay[j];
        q += ay[i] * ax[j];
    }
    return 0.5 * fabs(p - q);
}

__device__ void lm_iou(const lm_box& b1, const lm_box& b2, bool with_translation, double& iou, double& iou_2d) {
    const lm_corners c1 = lm_corners_of(b1, with_translation), c2 = lm_corners_of(b2, with_translation);
    const double a1 = lm_rect_area(c1), a2 = lm_rect_area(c2);
    const double inter = lm_clip_area(c1, c2);
    iou_2d = inter / (a1 + a2 - inter);
    const double ymax = c2.top < c1.top ? c2.top : c1.top;             // Python's min / max: the first argument unless the second beats it
    const double ymin = c2.bottom > c1.bottom ? c2.bottom : c1.bottom;
    const double dy = ymax - ymin;
    const double inter_vol = inter * (dy > 0.0 ? dy : 0.0);
    const double v1 = lm_vol(c1), v2 = lm_vol(c2);
    iou = inter_vol / (v2 < v1 ? v2 : v1);
}

// close_dis > 0.45 is "not close"; a NaN distance makes the reference's minimum NaN, which is not > 0.45
__device__ bool lm_close(const lm_box& s, const lm_box& o) {
    const lm_corners a = lm_corners_of(s, true), b = lm_corners_of(o, true);
    double best = INFINITY;
    bool nan = false;
    for (int i = 0; i < 8; ++i) {
        const double ax = a.x[i & 3], ay = i < 4 ? a.top : a.bottom, az = a.z[i & 3];
        for (int j = 0; j < 8; ++j) {
            const double dx = ax - b.x[j & 3], dy = ay - (j < 4 ? b.top : b.bottom), dz = az - b.z[j & 3];
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            nan |= d != d;
            best = d < best ? d : best;
        }
    }
    return nan || !(best > 0.45);
}

__device__ __forceinline__ float lm_l2(float p1x, float p1z, float p2x, float p2z) {
    const float dx = (p2x - p1x), dz = (p2z - p1z);
    return sqrtf(((dx * dx) + (dz * dz)));
}

__device__ bool lm_rule_ok(int rule, const lm_box& s, const lm_box& o, bool strict, double thr) {
    if (rule <= LM_BEHIND) {
        bool fail;
        if (rule == LM_LEFT) fail = (s.pz - o.pz) > -0.05f;
        else if (rule == LM_RIGHT) fail = (s.pz - o.pz) < 0.05f;
        else if (rule == LM_FRONT) fail = (s.px - o.px) < -0.05f;
        else fail = (s.px - o.px) > 0.05f;
        if (!fail && strict) {
            double iou, iou_2d;
            lm_iou(s, o, true, iou, iou_2d);
            fail = iou > thr;
        }
        return !fail;
    }
    if (rule == LM_SMALLER || rule == LM_BIGGER) {
        const float vs = ((s.l * s.h) * s.w), vo = ((o.l * o.h) * o.w);
        const float q = ((vs - vo) / vs);
        return rule == LM_BIGGER ? !(q < 0.15f) : !(q > -0.15f);
    }
    if (rule == LM_SHORTER || rule == LM_TALLER) {
        const float hs = (s.py + s.h), ho = (o.py + o.h);
        const float q = ((hs - ho) / hs);
        return rule == LM_TALLER ? !(q < 0.1f) : !(q > -0.1f);
    }
    if (rule == LM_STAND) return fabsf((s.py - o.py)) < 0.04f;
    if (rule == LM_CLOSE) return lm_close(s, o);
    return lm_l2(-s.px, -s.pz, o.px, o.pz) < 0.45f || lm_l2(-s.px, s.pz, o.px, o.pz) < 0.45f || lm_l2(s.px, -s.pz, o.px, o.pz) < 0.45f;
}

// keep[i] of the dtypes the mask may arrive in: 0 fp32, 1 int64, 2 one byte (bool, uint8, int8), 3 int32; as a double for == 0 / == 1
__device__ __forceinline__ double lm_keep(const void* keep, int dtype, long i) {
    if (dtype == 0) return (double)((const float*)keep)[i];
    if (dtype == 1) return (double)((const long*)keep)[i];
    if (dtype == 2) return (double)((const signed char*)keep)[i];
    return (double)((const int32_t*)keep)[i];
}

__global__ __launch_bounds__(LM_BLOCK) void k_relation_check(const float* boxes, int O, int ld, const long* triples, int T,
                                                             const signed char* rule_of_pred, int n_pred, const void* keep, int keep_dtype,
                                                             int keep_mode, int strict, double thr, signed char* rule_out,
                                                             signed char* ok_out, int32_t* counts, int32_t* status) {
    __shared__ int32_t sh[2 * LM_RULES];
    if (counts) {
        if (threadIdx.x < 2 * LM_RULES) sh[threadIdx.x] = 0;
        __syncthreads();
    }
    const long t = (long)blockIdx.x * LM_BLOCK + threadIdx.x;
    if (t < T) {
        const long s = triples[3 * t], p = triples[3 * t + 1], o = triples[3 * t + 2];
        int rule = -1, ok = 0, bad = 0;
        if (s < 0 || s >= O || o < 0 || o >= O) bad |= 1;
        if (p < 0 || p >= n_pred) bad |= 2;
        if (bad) atomicOr(status, bad);
        else {
            bool take = true;
            if (keep && keep_mode != 0) {
                const double ks = lm_keep(keep, keep_dtype, s), ko = lm_keep(keep, keep_dtype, o);
                take = keep_mode == 1 ? (ks == 1.0 && ko == 1.0) : (ks == 0.0 || ko == 0.0);
            }
            const int r = rule_of_pred[p];
            if (take && r >= 0 && r < LM_RULES) {
                rule = r;
                ok = lm_rule_ok(r, lm_load(boxes + s * ld), lm_load(boxes + o * ld), strict != 0, thr) ? 1 : 0;
                if (counts) {
                    atomicAdd(&sh[2 * r + 1], 1);
                    if (ok) atomicAdd(&sh[2 * r], 1);
                }
            }
        }
        rule_out[t] = (signed char)rule;
        ok_out[t] = (signed char)ok;
    }
    if (counts) {
        __syncthreads();
        if (threadIdx.x < 2 * LM_RULES && sh[threadIdx.x] != 0) atomicAdd(&counts[threadIdx.x], sh[threadIdx.x]);
    }
}

__global__ __launch_bounds__(LM_BLOCK) void k_box3d_iou(const float* a, int lda, const float* b, int ldb, int K, int with_translation,
                                                        double* iou, double* iou_2d) {
    const long k = (long)blockIdx.x * LM_BLOCK + threadIdx.x;
    if (k >= K) return;
    double v, v2;
    lm_iou(lm_load(a + k * lda), lm_load(b + k * ldb), with_translation != 0, v, v2);
    iou[k] = v;
    iou_2d[k] = v2;
}

}  // namespace

extern "C" int es_relation_check(const float* boxes, int O, int ld, const int64_t* triples, int T, const int8_t* rule_of_pred, int n_pred,
                                 const void* keep, int keep_dtype, int keep_mode, int strict, double overlap_threshold, int8_t* rule,
                                 int8_t* ok, int32_t* counts, int32_t* status, es_stream stream) {
    ES_REQUIRE(boxes && triples && rule_of_pred && rule && ok && status,
               "es_relation_check: NULL pointer (boxes %p triples %p rule_of_pred %p rule %p ok %p status %p)", (const void*)boxes,
               (const void*)triples, (const void*)rule_of_pred, (void*)rule, (void*)ok, (void*)status);
    ES_REQUIRE(O > 0 && ld >= 6 && T > 0 && n_pred > 0, "es_relation_check: O = %d boxes of ld = %d (>= 6), T = %d triples, n_pred = %d (all at least 1)",
               O, ld, T, n_pred);
    ES_REQUIRE(T <= 2147483647 - LM_BLOCK, "es_relation_check: T = %d triples are beyond the launch grid", T);
    ES_REQUIRE(keep_mode >= 0 && keep_mode <= 2, "es_relation_check: keep_mode = %d (0 every triple, 1 both ends kept, 2 an end not kept)", keep_mode);
    ES_REQUIRE(!keep || (keep_dtype >= 0 && keep_dtype <= 3), "es_relation_check: keep_dtype = %d (0 fp32, 1 int64, 2 one byte, 3 int32)", keep_dtype);
    ES_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
    if (counts) ES_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * LM_RULES * sizeof(int32_t), (hipStream_t)stream));
    hipLaunchKernelGGL(k_relation_check, dim3((unsigned)((T + LM_BLOCK - 1) / LM_BLOCK)), dim3(LM_BLOCK), 0, (hipStream_t)stream, boxes, O, ld,
                       (const long*)triples, T, (const signed char*)rule_of_pred, n_pred, keep, keep_dtype, keep_mode, strict ? 1 : 0,
                       overlap_threshold, (signed char*)rule, (signed char*)ok, counts, status);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_box3d_iou(const float* a, int lda, const float* b, int ldb, int K, int with_translation, double* iou, double* iou_2d,
                            es_stream stream) {
    ES_REQUIRE(a && b && iou && iou_2d, "es_box3d_iou: NULL pointer (a %p b %p iou %p iou_2d %p)", (const void*)a, (const void*)b, (void*)iou,
               (void*)iou_2d);
    ES_REQUIRE(K > 0 && lda >= 6 && ldb >= 6, "es_box3d_iou: K = %d pairs (at least 1) of rows with lda = %d, ldb = %d (>= 6)", K, lda, ldb);
    ES_REQUIRE(K <= 2147483647 - LM_BLOCK, "es_box3d_iou: K = %d pairs are beyond the launch grid", K);
    hipLaunchKernelGGL(k_box3d_iou, dim3((unsigned)((K + LM_BLOCK - 1) / LM_BLOCK)), dim3(LM_BLOCK), 0, (hipStream_t)stream, a, lda, b, ldb, K,
                       with_translation ? 1 : 0, iou, iou_2d);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
