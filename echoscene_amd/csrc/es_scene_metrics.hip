// Scene metrics: the point-cloud overlap between placed objects of the reference's helpers/metrics_3dfront.py (pointcloud_overlap,
// pointcloud_overlap_pair) with the fit of helpers/util.py (fit_shapes_to_box).  The reference fits, concatenates and builds a kd-tree
// per pair on the host; here a whole test set is three launches.
//
//   k_cloud_fit     : one workgroup per object.  Per axis min and max over the cloud (a fixed-order tree in LDS, no float atomics),
//                     then every point: p / size * box[:3], the rotation by box[6] degrees, + box[3:6]; the placed cloud and its
//                     axis-aligned bounds (lo x, y, z, hi x, y, z: again a tree, over the values as written) go out.  Without boxes
//                     the cloud is taken as placed: bounds and the finiteness check only.
//   k_cloud_self_nn : one lane per query point, its own cloud streamed through LDS as float4, one broadcast ds_read_b128 per
//                     candidate (the structure of k_chamfer_nn): d11 = the squared distance to the nearest point of another index,
//                     +inf for P = 1.  Once per object, where every pair of the reference rebuilds it inside its kd-tree.
//   k_cloud_overlap : grid (pairs, query chunks).  A lane holds one query of the first cloud and its radius d11 and is finished when it
//                     has met a point of the second cloud with d < d11 (it counts) or when its squared distance to the bounds of the
//                     second cloud is already >= d11 (it cannot).  The workgroup leaves the tile loop when every lane is finished (one
//                     __syncthreads_or per LDS tile, the barrier the tile needs anyway).  Counts: ballots per wave, LDS, one integer
//                     atomicAdd per workgroup: integers, so a count does not depend on the order of arrival.
//
// Arithmetic: fp32, every operation rounded on its own (no contraction: the pragma below, plain operators).  The fit follows the
// reference per axis and in its order; the angle goes to radians in fp32 (a * fl(fl(pi) / 180), as numpy's deg2rad on a float32), and its
// cosine and sine are the correctly rounded fp32 values (evaluated in double, once per object, rounded once).  Distances are direct
// differences, dx*dx + dy*dy + dz*dz summed in that order, compared as squares.  The bounds test prunes nothing it should not: the
// rounded difference, square and sum are monotone, so the squared distance to the bounds, formed by the same operations in the same
// order, is <= the computed d of every point inside them.
//
// Status: k_cloud_fit writes a word per object (bit 0 an axis of zero extent, bit 1 a value that is not finite: a coordinate, a
// box entry, a size quotient); k_cloud_overlap raises bit 0 of one word for a pair index out of range, and reads nothing through it.

#pragma clang fp contract(off)

#include "es_common.h"

namespace {

constexpr int SM_BLOCK = 256;
constexpr int SM_TILE = 2048;                  // candidates per LDS tile: 32 KB as float4
constexpr int SM_CHUNK = 64;                   // candidates between two looks at whether the wave is finished

__device__ __forceinline__ bool sm_finite(float v) { return (v - v) == 0.0f; }

// min / max of six values per thread over the workgroup, in a fixed order; the result is in sh[0..5] for every thread after the call
__device__ __forceinline__ void sm_reduce_bounds(float (*sh)[SM_BLOCK], float lo[3], float hi[3]) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) { sh[c][t] = lo[c]; sh[3 + c][t] = hi[c]; }
    __syncthreads();
    for (int s = SM_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sh[c][t] = fminf(sh[c][t], sh[c][t + s]);
                sh[3 + c][t] = fmaxf(sh[3 + c][t], sh[3 + c][t + s]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = sh[c][0]; hi[c] = sh[3 + c][0]; }
}

__global__ __launch_bounds__(SM_BLOCK) void k_cloud_fit(const float* clouds, int P, const float* boxes, int ld, int withangle, int up_y,
                                                        float* placed, float* bounds, int32_t* status) {
    __shared__ float sh[6][SM_BLOCK];
    __shared__ int32_t sh_status;
    const int o = blockIdx.x, t = threadIdx.x;
    const float* src = clouds + (long)o * P * 3;
    if (t == 0) sh_status = 0;
    int bad = 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int p = t; p < P; p += SM_BLOCK) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = src[3 * p + c];
            if (!sm_finite(v)) bad |= 2;
            lo[c] = fminf(lo[c], v);
            hi[c] = fmaxf(hi[c], v);
        }
    }
    sm_reduce_bounds(sh, lo, hi);
    if (boxes) {
        const float* box = boxes + (long)o * ld;
        float size[3], scale[3], shift[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            size[c] = (hi[c] - lo[c]);
            scale[c] = box[c];
            shift[c] = box[3 + c];
            if (size[c] == 0.0f) bad |= 1;
            if (!sm_finite(scale[c]) || !sm_finite(shift[c])) bad |= 2;
        }
        float cs = 1.0f, sn = 0.0f;
        if (withangle) {
            const float rad = (box[6] * (3.14159265358979323846f / 180.0f));
            if (!sm_finite(rad)) bad |= 2;
            else { cs = (float)cos((double)rad); sn = (float)sin((double)rad); }
        }
        float* dst = placed + (long)o * P * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = INFINITY; hi[c] = -INFINITY; }
        const int a = 0, b = up_y ? 2 : 1;                              // the two axes that turn
        for (int p = t; p < P; p += SM_BLOCK) {
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = ((src[3 * p + c] / size[c]) * scale[c]);
            if (withangle) {
                const float u = ((cs * v[a]) - (sn * v[b])), w = ((sn * v[a]) + (cs * v[b]));
                v[a] = u;
                v[b] = w;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = (v[c] + shift[c]);
                if (!sm_finite(v[c])) bad |= 2;
                dst[3 * p + c] = v[c];
                lo[c] = fminf(lo[c], v[c]);
                hi[c] = fmaxf(hi[c], v[c]);
            }
        }
        sm_reduce_bounds(sh, lo, hi);
    }
    if (bad) atomicOr(&sh_status, bad);
    __syncthreads();
    if (t < 3) { bounds[6 * o + t] = lo[t]; bounds[6 * o + 3 + t] = hi[t]; }
    if (t == 0) status[o] = sh_status;
}

__global__ __launch_bounds__(SM_BLOCK) void k_cloud_self_nn(const float* clouds, int P, float* d11) {
    __shared__ f4 buf[SM_TILE];
    const int o = blockIdx.x;
    const int j = blockIdx.y * SM_BLOCK + threadIdx.x;
    const float* base = clouds + (long)o * P * 3;
    const float* q = base + 3 * (j < P ? j : 0);
    const float x1 = q[0], y1 = q[1], z1 = q[2];
    float best = INFINITY;
    for (int k2 = 0; k2 < P; k2 += SM_TILE) {
        const int cnt = min(SM_TILE, P - k2);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += SM_BLOCK) {
            const float* p = base + 3 * (k2 + t);
            buf[t] = f4{p[0], p[1], p[2], 0.f};
        }
        __syncthreads();
        const int self = j - k2;                                        // the lane's own point, if it is in this tile
        for (int k = 0; k < cnt; ++k) {
            const f4 p = buf[k];
            const float dx = (p[0] - x1), dy = (p[1] - y1), dz = (p[2] - z1);
            const float d = (((dx * dx) + (dy * dy)) + (dz * dz));
            if (k != self && d < best) best = d;
        }
    }
    if (j < P) d11[(long)o * P + j] = best;
}

__global__ __launch_bounds__(SM_BLOCK) void k_cloud_overlap(const float* qclouds, int Oq, int Pq, const float* d11, const float* cclouds,
                                                            int Oc, int Pc, const float* cbounds, const int32_t* pairs, int32_t* counts,
                                                            int32_t* status) {
    __shared__ f4 buf[SM_TILE];
    __shared__ int32_t sh_count;
    const int k = blockIdx.x;
    const int i = pairs[2 * k], j2 = pairs[2 * k + 1];
    if (i < 0 || i >= Oq || j2 < 0 || j2 >= Oc) {                       // the same for the whole workgroup: nothing is read through it
        if (threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    if (threadIdx.x == 0) sh_count = 0;
    const int j = blockIdx.y * SM_BLOCK + threadIdx.x;
    const float* q = qclouds + ((long)i * Pq + (j < Pq ? j : 0)) * 3;
    const float x1 = q[0], y1 = q[1], z1 = q[2];
    const float r = d11[(long)i * Pq + (j < Pq ? j : 0)];
    const float* cb = cbounds + 6 * (long)j2;
    // squared distance to the bounds of the second cloud, by the operations of a candidate's distance
    const float bx = x1 < cb[0] ? (cb[0] - x1) : (x1 > cb[3] ? (cb[3] - x1) : 0.0f);
    const float by = y1 < cb[1] ? (cb[1] - y1) : (y1 > cb[4] ? (cb[4] - y1) : 0.0f);
    const float bz = z1 < cb[2] ? (cb[2] - z1) : (z1 > cb[5] ? (cb[5] - z1) : 0.0f);
    const float dbox = (((bx * bx) + (by * by)) + (bz * bz));
    bool hit = false;
    bool done = j >= Pq || dbox >= r;
    const float* base = cclouds + (long)j2 * Pc * 3;
    for (int k2 = 0; k2 < Pc; k2 += SM_TILE) {
        if (!__syncthreads_or(done ? 0 : 1)) break;                     // also: every lane has left the previous tile
        const int cnt = min(SM_TILE, Pc - k2);
        for (int t = threadIdx.x; t < cnt; t += SM_BLOCK) {
            const float* p = base + 3 * (k2 + t);
            buf[t] = f4{p[0], p[1], p[2], 0.f};
        }
        __syncthreads();
        for (int c0 = 0; c0 < cnt; c0 += SM_CHUNK) {
            if (__all(done ? 1 : 0)) break;                             // the whole wave is finished
            const int c1 = min(cnt, c0 + SM_CHUNK);
            bool found = false;
            for (int c = c0; c < c1; ++c) {
                const f4 p = buf[c];
                const float dx = (p[0] - x1), dy = (p[1] - y1), dz = (p[2] - z1);
                const float d = (((dx * dx) + (dy * dy)) + (dz * dz));
                found |= d < r;
            }
            if (found && !done) { hit = true; done = true; }
        }
    }
    const int n = __popcll(__ballot(hit ? 1 : 0));
    __syncthreads();                                                    // sh_count is zero for everyone; the tile loop is left
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&sh_count, n);
    __syncthreads();
    if (threadIdx.x == 0 && sh_count) atomicAdd(&counts[k], sh_count);
}

}  // namespace

extern "C" int es_cloud_fit(const float* clouds, int O, int P, const float* boxes, int ld, int withangle, int up, float* placed,
                            float* bounds, int32_t* status, es_stream stream) {
    ES_REQUIRE(clouds && bounds && status, "es_cloud_fit: NULL pointer (clouds %p bounds %p status %p)", (const void*)clouds, (void*)bounds,
               (void*)status);
    ES_REQUIRE(O > 0 && P > 0, "es_cloud_fit: O = %d clouds of P = %d points (both at least 1)", O, P);
    ES_REQUIRE((long)O * P * 3 < 2147483647L, "es_cloud_fit: O * P * 3 = %ld is beyond int32 indexing", (long)O * P * 3);
    ES_REQUIRE(!boxes || (placed && ld >= (withangle ? 7 : 6)), "es_cloud_fit: boxes given with placed %p, ld = %d (>= %d)", (void*)placed, ld,
               withangle ? 7 : 6);
    ES_REQUIRE(up == 0 || up == 1, "es_cloud_fit: up = %d (0 the angle turns about z, 1 about y)", up);
    hipLaunchKernelGGL(k_cloud_fit, dim3((unsigned)O), dim3(SM_BLOCK), 0, (hipStream_t)stream, clouds, P, boxes, ld, withangle ? 1 : 0, up,
                       placed, bounds, status);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_cloud_self_nn(const float* clouds, int O, int P, float* d11, es_stream stream) {
    ES_REQUIRE(clouds && d11, "es_cloud_self_nn: NULL pointer (clouds %p d11 %p)", (const void*)clouds, (void*)d11);
    ES_REQUIRE(O > 0 && P > 0, "es_cloud_self_nn: O = %d clouds of P = %d points (both at least 1)", O, P);
    ES_REQUIRE((long)O * P * 3 < 2147483647L, "es_cloud_self_nn: O * P * 3 = %ld is beyond int32 indexing", (long)O * P * 3);
    hipLaunchKernelGGL(k_cloud_self_nn, dim3((unsigned)O, (unsigned)((P + SM_BLOCK - 1) / SM_BLOCK)), dim3(SM_BLOCK), 0, (hipStream_t)stream,
                       clouds, P, d11);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_cloud_overlap(const float* qclouds, int Oq, int Pq, const float* d11, const float* cclouds, int Oc, int Pc,
                                const float* cbounds, const int32_t* pairs, int K, int32_t* counts, int32_t* status, es_stream stream) {
    ES_REQUIRE(qclouds && d11 && cclouds && cbounds && pairs && counts && status,
               "es_cloud_overlap: NULL pointer (qclouds %p d11 %p cclouds %p cbounds %p pairs %p counts %p status %p)", (const void*)qclouds,
               (const void*)d11, (const void*)cclouds, (const void*)cbounds, (const void*)pairs, (void*)counts, (void*)status);
    ES_REQUIRE(Oq > 0 && Pq > 0 && Oc > 0 && Pc > 0, "es_cloud_overlap: Oq = %d clouds of Pq = %d points, Oc = %d of Pc = %d (all at least 1)", Oq,
               Pq, Oc, Pc);
    ES_REQUIRE(K > 0, "es_cloud_overlap: K = %d pairs (at least 1)", K);
    ES_REQUIRE((long)Oq * Pq * 3 < 2147483647L && (long)Oc * Pc * 3 < 2147483647L, "es_cloud_overlap: a cloud set of %ld or %ld floats is beyond int32 indexing",
               (long)Oq * Pq * 3, (long)Oc * Pc * 3);
    ES_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), (hipStream_t)stream));
    ES_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)K * sizeof(int32_t), (hipStream_t)stream));
    hipLaunchKernelGGL(k_cloud_overlap, dim3((unsigned)K, (unsigned)((Pq + SM_BLOCK - 1) / SM_BLOCK)), dim3(SM_BLOCK), 0, (hipStream_t)stream,
                       qclouds, Oq, Pq, d11, cclouds, Oc, Pc, cbounds, pairs, counts, status);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
