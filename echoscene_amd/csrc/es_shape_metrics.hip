// Shape-set metrics (the end of the path SDF -> mesh -> point cloud -> distance matrix): the matrix of
// Chamfer distances between every cloud of one set and every cloud of another, which MMD, COV and 1-NN accuracy of the reference's
// scripts/compute_mmd_cov_1nn.py are statistics of, and the point-cloud preparation in front of it (its sample_pc + normalization).
// The reference expands one cloud against a batch of the others and calls its per-point Chamfer kernel (_pairwise_EMD_CD_), which
// returns a distance and an index per point; the matrix needs a minimum and a mean only.
//
//   k_chamfer_matrix  : one workgroup of 256 threads per pair (i, j), both directions, out[i, j] written once: no atomics, no partial
//                       results across workgroups, so an entry's bits depend on the two clouds alone -- not on the run, not on the other
//                       clouds of the call, and not on the order of the arguments (the two directions are the same two sums, added in
//                       double, and addition commutes).
//   k_cloud_normalize : one workgroup per cloud: gather `number` vertices by index, subtract their mean, divide by the largest absolute
//                       coordinate of the centred cloud; everything in double, rounded to float once.
//
// Distances: the expanded form of the reference's own distChamfer (xx + yy - 2 zz in fp32) on the exact-fp32 matrix instruction,
// v_mfma_f32_16x16x4_f32 with K = 4: the A operand of a lane is component k = lane >> 4 of query lane & 15, (x0, x1, x2, 1); the B
// operand is component k of candidate lane & 15, (-2 y0, -2 y1, -2 y2, |y|^2), prepared while the candidates are staged into LDS.  The
// result is the fmaf chain fma(1, |y|^2, fma(x2, -2 y2, fma(x1, -2 y1, x0 * -2 y0))) with the candidate on the lane (column lane & 15)
// and query 4 (lane >> 4) + r in register r.  256 distances per instruction; the VALU adds one v_min3 per two distances.  |x|^2 does not depend
// on the candidate and is added after the minimum.  The form cancels for coordinates far from the origin: the contract is clouds
// normalised as the reference normalises them (centred, max |coordinate| = 1), which k_cloud_normalize produces.
//
// Tiling: a wave keeps CM_QT = 4 tiles of 16 queries (four independent accumulators: the instruction issues every 32 cycles and
// returns after 40), the four waves of a workgroup take CM_PASS = 256 queries per pass.  The candidates are staged in chunks of
// CM_CHUNK = 2048 points (32 KiB of float4: five workgroups per CU); running minima are element-wise per accumulator register and
// persist over the chunks of a pass; a cloud of one chunk is staged once for all passes.  Tails: candidates are padded to a pair of
// 16-point tiles with (0, 0, 0, CM_FAR), which can never win; padded queries compute on zeros and are left out of the sum; no load goes past a
// cloud.  At the end of a pass the minima are reduced over the 16 lanes of a row, each lane takes one query, adds |x|^2, clamps at 0
// (the expanded form can return about -1e-7 for a coincident pair; the reference does not clamp) and adds to its double accumulator.
// Sums run in a fixed order: per lane over the passes, a fixed tree over the lanes of a wave, then the waves in index order.
#include "es_common.h"

namespace {

constexpr int CM_BLOCK = 256;
constexpr int CM_QT = 4;                       // 16-query tiles per wave
constexpr int CM_WQ = 16 * CM_QT;              // queries per wave and pass
constexpr int CM_PASS = (CM_BLOCK / 64) * CM_WQ;
constexpr int CM_CHUNK = 2048;                 // candidates per LDS stage
constexpr float CM_FAR = 1e30f;                // |y|^2 of a padding candidate: finite, beyond any real distance

// min(a, b) as med3(a, b, -inf); the compiler folds two of them into one v_min3_f32.  fminf is the IEEE minNum, which quiets a signalling
// NaN first: a v_max_f32 x, x on each operand, three VALU instructions per distance where the matrix unit leaves room for one.  No NaN
// handling is wanted here.
__device__ __forceinline__ float cm_min(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, -INFINITY); }

__device__ __forceinline__ long cm_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sum over the queries x[0 .. nq) of max(min over the candidates y[0 .. ny) of |x - y|^2, 0); the same value in every thread
__device__ __forceinline__ double cm_direction(const float* __restrict__ x, int nq, const float* __restrict__ y, int ny, f4* cand,
                                               double* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, k = lane >> 4;
    const int nchunk = (ny + CM_CHUNK - 1) / CM_CHUNK;
    const float* candf = (const float*)cand;
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    double acc = 0.0;
    for (int q0 = 0; q0 < nq; q0 += CM_PASS) {
        const int qw = q0 + wave * CM_WQ;
        float a[CM_QT];
        f4 best[CM_QT];
#pragma unroll
        for (int t = 0; t < CM_QT; ++t) {
            const int q = qw + 16 * t + col;
            a[t] = k == 3 ? 1.f : (q < nq ? x[3 * (long)q + k] : 0.f);
            best[t] = f4{CM_FAR, CM_FAR, CM_FAR, CM_FAR};
        }
        for (int c = 0; c < nchunk; ++c) {
            const int c0 = c * CM_CHUNK;
            const int cnt = min(CM_CHUNK, ny - c0);
            if (nchunk > 1 || q0 == 0) {                            // (uniform over the workgroup)
                __syncthreads();
                const int padded = (cnt + 31) & ~31;
                for (int t = threadIdx.x; t < padded; t += CM_BLOCK) {
                    f4 v = {0.f, 0.f, 0.f, CM_FAR};
                    if (t < cnt) {
                        const float* p = y + 3 * (long)(c0 + t);
                        const float y0 = p[0], y1 = p[1], y2 = p[2];
                        v = f4{-2.f * y0, -2.f * y1, -2.f * y2, __fmaf_rn(y2, y2, __fmaf_rn(y1, y1, y0 * y0))};
                    }
                    cand[t] = v;
                }
                __syncthreads();
            }
            if (qw < nq) {                                          // (uniform over the wave; a wave without queries only keeps the barriers)
                const int pairs = (cnt + 31) >> 5;                  // two candidate tiles per round: eight products in flight
                for (int tl = 0; tl < pairs; ++tl) {
                    const float b0 = candf[(tl * 32 + col) * 4 + k], b1 = candf[(tl * 32 + 16 + col) * 4 + k];
#pragma unroll
                    for (int t = 0; t < CM_QT; ++t) {
                        const f4 d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b0, zero, 0, 0, 0);
                        const f4 d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b1, zero, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) best[t][r] = cm_min(cm_min(best[t][r], d0[r]), d1[r]);
                    }
                }
            }
        }
        // the minimum over the 16 candidate columns of a row; lane `col` of each row group then takes register (col >> 2, col & 3)
        float mine = 0.f;
#pragma unroll
        for (int t = 0; t < CM_QT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = best[t][r];
                v = fminf(v, __shfl_xor(v, 1));
                v = fminf(v, __shfl_xor(v, 2));
                v = fminf(v, __shfl_xor(v, 4));
                v = fminf(v, __shfl_xor(v, 8));
                if (col == 4 * t + r) mine = v;
            }
        const int q = qw + 16 * (col >> 2) + 4 * k + (col & 3);
        if (q < nq) {
            const float* p = x + 3 * (long)q;
            const float x0 = p[0], x1 = p[1], x2 = p[2];
            const float xx = __fmaf_rn(x2, x2, __fmaf_rn(x1, x1, x0 * x0));
            acc += (double)fmaxf(mine + xx, 0.f);
        }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) acc += __shfl_down(acc, w);
    __syncthreads();                                                // (part of the previous direction has been read by everyone)
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(CM_BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void k_chamfer_matrix(const float* a, int P, const float* b, int Nb, int Q, int symmetric,
                                                             float* out) {
    __shared__ f4 cand[CM_CHUNK];
    double* part = (double*)cand;                                   // (the wave sums of a direction, after its last read of the candidates)
    const int i = (int)(blockIdx.x / (unsigned)Nb), j = (int)(blockIdx.x % (unsigned)Nb);
    if (symmetric) {                                                // pairs with i < j, mirrored; the diagonal is exactly 0
        if (i > j) return;
        if (i == j) {
            if (threadIdx.x == 0) out[(long)i * Nb + j] = 0.f;
            return;
        }
    }
    const float* ai = a + (long)i * P * 3;
    const float* bj = b + (long)j * Q * 3;
    const double s1 = cm_direction(ai, P, bj, Q, cand, part);
    const double s2 = cm_direction(bj, Q, ai, P, cand, part);
    if (threadIdx.x == 0) {
        const float v = (float)(s1 / (double)P + s2 / (double)Q);
        out[(long)i * Nb + j] = v;
        if (symmetric) out[(long)j * Nb + i] = v;
    }
}

__global__ __launch_bounds__(CM_BLOCK) void k_cloud_normalize(const float* verts, const long* vofs, long total_V, const int32_t* index,
                                                              int number, float* out, int32_t* bad) {
    __shared__ double sh[3][CM_BLOCK];
    const int k = blockIdx.x, tid = threadIdx.x;
    const long v0 = cm_clampl(vofs[k], 0, total_V), vn = cm_clampl(vofs[k + 1], v0, total_V) - v0;
    const int32_t* idx = index + (long)k * number;
    float* o = out + (long)k * number * 3;
    if (vn <= 0) {                                                  // a cloud without vertices: nothing to gather (uniform)
        for (int p = tid; p < 3 * number; p += CM_BLOCK) o[p] = 0.f;
        if (tid == 0) bad[k] = 1;
        return;
    }
    const float* v = verts + 3 * v0;
    int flag = 0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int p = tid; p < number; p += CM_BLOCK) {
        long id = idx[p];
        if (id < 0 || id >= vn) {                                   // flagged and clamped, never dereferenced as given
            flag = 1;
            id = cm_clampl(id, 0, vn - 1);
        }
        for (int c = 0; c < 3; ++c) s[c] += (double)v[3 * id + c];
    }
    for (int c = 0; c < 3; ++c) sh[c][tid] = s[c];
    flag = __syncthreads_or(flag);
    for (int w = CM_BLOCK / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int c = 0; c < 3; ++c) sh[c][tid] += sh[c][tid + w];
        __syncthreads();
    }
    const double mean[3] = {sh[0][0] / number, sh[1][0] / number, sh[2][0] / number};
    __syncthreads();
    double mx = 0.0;
    for (int p = tid; p < number; p += CM_BLOCK) {
        const long id = cm_clampl(idx[p], 0, vn - 1);
        for (int c = 0; c < 3; ++c) mx = fmax(mx, fabs((double)v[3 * id + c] - mean[c]));
    }
    sh[0][tid] = mx;
    __syncthreads();
    for (int w = CM_BLOCK / 2; w > 0; w >>= 1) {
        if (tid < w) sh[0][tid] = fmax(sh[0][tid], sh[0][tid + w]);
        __syncthreads();
    }
    mx = sh[0][0];
    for (int p = tid; p < number; p += CM_BLOCK) {
        const long id = cm_clampl(idx[p], 0, vn - 1);
        for (int c = 0; c < 3; ++c) o[3 * p + c] = (float)(((double)v[3 * id + c] - mean[c]) / mx);    // all points equal: 0 / 0 = NaN
    }
    if (tid == 0) bad[k] = flag ? 1 : 0;
}

}  // namespace

extern "C" int es_chamfer_matrix(const float* a, int Na, int P, const float* b, int Nb, int Q, int symmetric, float* out,
                                 es_stream stream) {
    ES_REQUIRE(a && b && out, "es_chamfer_matrix: NULL pointer (a %p b %p out %p)", (const void*)a, (const void*)b, (void*)out);
    ES_REQUIRE(Na > 0 && Nb > 0 && P > 0 && Q > 0, "es_chamfer_matrix: empty clouds (Na=%d P=%d Nb=%d Q=%d)", Na, P, Nb, Q);
    ES_REQUIRE((long)Na * P * 3 <= 2147483647L && (long)Nb * Q * 3 <= 2147483647L,
               "es_chamfer_matrix: %d x %d x 3 or %d x %d x 3 coordinates are beyond int32 indexing", Na, P, Nb, Q);
    ES_REQUIRE((long)Na * Nb <= 2147483647L, "es_chamfer_matrix: %d x %d pairs are beyond int32 indexing", Na, Nb);
    ES_REQUIRE(!symmetric || (b == a && Nb == Na && Q == P),
               "es_chamfer_matrix: symmetric needs b == a with the same counts (a %p [%d, %d, 3], b %p [%d, %d, 3])", (const void*)a, Na, P,
               (const void*)b, Nb, Q);
    hipLaunchKernelGGL(k_chamfer_matrix, dim3((unsigned)(Na * Nb)), dim3(CM_BLOCK), 0, (hipStream_t)stream, a, P, b, Nb, Q,
                       symmetric ? 1 : 0, out);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_cloud_normalize(const float* verts, const int64_t* vert_offset, const int32_t* index, int K, int number, long total_V,
                                  int32_t* bad_flags, float* out, es_stream stream) {
    ES_REQUIRE(verts && vert_offset && index && bad_flags && out,
               "es_cloud_normalize: NULL pointer (verts %p vert_offset %p index %p bad_flags %p out %p)", (const void*)verts,
               (const void*)vert_offset, (const void*)index, (void*)bad_flags, (void*)out);
    ES_REQUIRE(K > 0 && number > 0, "es_cloud_normalize: K = %d clouds of number = %d points (both at least 1)", K, number);
    ES_REQUIRE((long)K * number * 3 <= 2147483647L, "es_cloud_normalize: %d x %d x 3 coordinates are beyond int32 indexing", K, number);
    ES_REQUIRE(total_V >= 0 && total_V <= 2147483647L / 3, "es_cloud_normalize: total_V = %ld is beyond int32 indexing (0 .. %ld)", total_V,
               2147483647L / 3);
    hipLaunchKernelGGL(k_cloud_normalize, dim3(K), dim3(CM_BLOCK), 0, (hipStream_t)stream, verts, (const long*)vert_offset, total_V, index,
                       number, out, bad_flags);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
