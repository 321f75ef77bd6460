// Triangle meshes -> truncated signed distance grids on the device: the inverse of es_mc.hip, so that a caller with a mesh (a dataset
// model, a scan, a mesh sdf_to_mesh returned) gets the [K, n, n, n] grids the shape-keeping and shape-completing calls take.  The
// reference only reads precomputed grids (dataset/threedfront_dataset.py:313-317, clamped to +-0.2); the tool that made them is not
// part of it, so the arithmetic below is this package's own: the exact point-triangle distance and the generalized winding number
// (Jacobson et al. 2013; the solid angle of a triangle by van Oosterom & Strackee 1983), brute force over all triangles.
//
// Grid convention (the inverse of postprocess.sdf_to_mesh): voxel (i, j, k) is the point (i/n - 0.5, j/n - 0.5, k/n - 0.5), array axes
// are x, y, z, negative is inside, the value is clamp(+-distance, -trunc, trunc).
//
//   k_ms_frame : one workgroup per mesh: the bounding box of its vertices -> centre and scale of the fit (identity without a fit), in
//                double into the workspace and in float to the caller; clears the mesh's bad-index flag.
//   k_ms_prep  : one thread per triangle: gathers the three vertices (a face index outside the mesh is clamped and raises the flag),
//                applies the fit in double (one rounding per coordinate) and writes one 36-float record: the vertices, the unit normal,
//                per edge the unit direction, the length and the in-plane unit normal pointing into the triangle, twice the area, and
//                a skip mark for a triangle of zero area.  Everything that is a quotient of differences is formed in double here, so a
//                thin triangle's normal is as good as a fat one's.
//   k_ms_grid  : grid (256-voxel blocks, K), a thread owns a voxel.  Records stream through LDS in tiles of MS_TILE; all lanes read
//                the same record (broadcast reads), so every select below is per lane and no branch diverges.  Each thread keeps the
//                minimum squared distance and the sum of the half solid angles over the triangles in their order: no atomics, the same
//                bits on every run, and a mesh's grid does not depend on what else is in the batch.
//
// Distance: with a, b, c the vectors from the voxel P to the corners, the closest point Q of the triangle is the foot of the
// perpendicular when P projects into the triangle (its three in-plane edge coordinates say so) and the nearest point of the three
// edge segments otherwise; the squared distance is |Q - P|^2 of the vector itself (never |AP|^2 - projection^2, which cancels next to
// the surface).  Sign: w = (1 / 2 pi) sum atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), inside when w > 0.5; the
// numerator a . (b x c) equals (a . n) * (twice the area), which the plane term has already.
#include "es_common.h"

namespace {

constexpr int MS_BLOCK = 256;
constexpr int MS_TILE = 128;             // triangles per LDS tile: 18 KiB, 8 workgroups per CU stay resident
constexpr int MS_REC = 9;                // float4 per record

struct d3 { double x, y, z; };
__device__ __forceinline__ d3 operator-(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ d3 scaled(d3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// frame[m] = {centre x, y, z, scale}: fitted = (v - centre) * scale
__global__ __launch_bounds__(MS_BLOCK) void k_ms_frame(const float* verts, const long* vofs, long total_V, float fit, double* frame,
                                                       float* transform, int32_t* bad) {
    __shared__ float sh[6][MS_BLOCK];
    const int m = blockIdx.x;
    const long v0 = clampl(vofs[m], 0, total_V), v1 = clampl(vofs[m + 1], v0, total_V);
    double c[3] = {0.0, 0.0, 0.0}, s = 1.0;
    if (fit > 0.f && v1 > v0) {                                     // (uniform over the workgroup)
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (long v = v0 + threadIdx.x; v < v1; v += MS_BLOCK)
            for (int a = 0; a < 3; ++a) {
                const float x = verts[3 * v + a];
                lo[a] = fminf(lo[a], x);
                hi[a] = fmaxf(hi[a], x);
            }
        for (int a = 0; a < 3; ++a) { sh[a][threadIdx.x] = lo[a]; sh[3 + a][threadIdx.x] = hi[a]; }
        __syncthreads();
        for (int w = MS_BLOCK / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w)
                for (int a = 0; a < 3; ++a) {
                    sh[a][threadIdx.x] = fminf(sh[a][threadIdx.x], sh[a][threadIdx.x + w]);
                    sh[3 + a][threadIdx.x] = fmaxf(sh[3 + a][threadIdx.x], sh[3 + a][threadIdx.x + w]);
                }
            __syncthreads();
        }
        double side = 0.0;
        for (int a = 0; a < 3; ++a) {
            c[a] = 0.5 * ((double)sh[a][0] + (double)sh[3 + a][0]);
            side = fmax(side, (double)sh[3 + a][0] - (double)sh[a][0]);
        }
        if (side > 0.0 && side < (double)INFINITY) s = (double)fit / side;      // (a single point keeps its scale)
    }
    if (threadIdx.x == 0) {
        for (int a = 0; a < 3; ++a) frame[4 * m + a] = c[a];
        frame[4 * m + 3] = s;
        if (transform) {
            for (int a = 0; a < 3; ++a) transform[4 * m + a] = (float)c[a];
            transform[4 * m + 3] = (float)s;
        }
        bad[m] = 0;
    }
}

__global__ __launch_bounds__(MS_BLOCK) void k_ms_prep(const float* verts, const int32_t* faces, const long* vofs, const long* tofs, int K,
                                                      long total_V, long total_T, const double* frame, float4* rec, int32_t* bad) {
    const long t = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t >= total_T) return;
    int lo = 0, hi = K - 1;                                         // the mesh of triangle t: the last m with tofs[m] <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tofs[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int m = lo;
    const long vb = clampl(vofs[m], 0, total_V), vn = clampl(vofs[m + 1], vb, total_V) - vb;
    float4* r = rec + t * MS_REC;
    const float4 zero = {0.f, 0.f, 0.f, 0.f};
    bool skip = vn <= 0;
    d3 P[3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (skip) {
        bad[m] = 1;                                                 // faces of a mesh without vertices
    } else {
        const double cx = frame[4 * m], cy = frame[4 * m + 1], cz = frame[4 * m + 2], s = frame[4 * m + 3];
        for (int e = 0; e < 3; ++e) {
            long id = faces[3 * t + e];
            if (id < 0 || id >= vn) {
                bad[m] = 1;
                id = clampl(id, 0, vn - 1);
            }
            const float* v = verts + 3 * (vb + id);
            // the fitted corner, rounded to float once: the grid kernel and every quantity below see the same triangle
            P[e] = {(double)(float)(((double)v[0] - cx) * s), (double)(float)(((double)v[1] - cy) * s), (double)(float)(((double)v[2] - cz) * s)};
        }
    }
    const d3 ab = P[1] - P[0], bc = P[2] - P[1], ca = P[0] - P[2];
    const double l2ab = dot(ab, ab), l2bc = dot(bc, bc), l2ca = dot(ca, ca);
    const d3 N = cross(ab, scaled(ca, -1.0));                       // AB x AC
    const double area2 = sqrt(dot(N, N)), l2max = fmax(l2ab, fmax(l2bc, l2ca));
    // zero area: three equal or collinear corners (in double the products of float differences are nearly exact; what is left of a
    // collinear triple is far below this bar, and a real sliver far above it).  Not finite: skipped as well.
    if (!(area2 > 1e-12 * l2max) || !(l2max < (double)INFINITY)) skip = true;
    if (skip) {
        for (int q = 0; q < MS_REC; ++q) r[q] = zero;
        r[7].w = 1.f;
        return;
    }
    const d3 n = scaled(N, 1.0 / area2);
    const double lab = sqrt(l2ab), lbc = sqrt(l2bc), lca = sqrt(l2ca);
    const d3 uab = scaled(ab, 1.0 / lab), ubc = scaled(bc, 1.0 / lbc), uca = scaled(ca, 1.0 / lca);
    const d3 mab = cross(n, uab), mbc = cross(n, ubc), mca = cross(n, uca);     // in the plane, towards the inside
    r[0] = {(float)P[0].x, (float)P[0].y, (float)P[0].z, (float)n.x};
    r[1] = {(float)P[1].x, (float)P[1].y, (float)P[1].z, (float)n.y};
    r[2] = {(float)P[2].x, (float)P[2].y, (float)P[2].z, (float)n.z};
    r[3] = {(float)mab.x, (float)mab.y, (float)mab.z, (float)lab};
    r[4] = {(float)mbc.x, (float)mbc.y, (float)mbc.z, (float)lbc};
    r[5] = {(float)mca.x, (float)mca.y, (float)mca.z, (float)lca};
    r[6] = {(float)uab.x, (float)uab.y, (float)uab.z, (float)area2};
    r[7] = {(float)ubc.x, (float)ubc.y, (float)ubc.z, 0.f};
    r[8] = {(float)uca.x, (float)uca.y, (float)uca.z, 0.f};
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __fmaf_rn(az, bz, __fmaf_rn(ay, by, ax * bx));
}

// |(x, y, z)| for the winding term only (the distance takes one correctly rounded sqrtf per voxel, at the end)
__device__ __forceinline__ float es_ms_len(float x, float y, float z) { return __builtin_amdgcn_sqrtf(dot3(x, y, z, x, y, z)); }

// squared distance from the origin to the segment that starts at (px, py, pz), runs along the unit vector u and is `len` long
__device__ __forceinline__ float seg_d2(float px, float py, float pz, float4 u, float len) {
    const float s = fminf(fmaxf(-dot3(px, py, pz, u.x, u.y, u.z), 0.f), len);
    const float qx = __fmaf_rn(s, u.x, px), qy = __fmaf_rn(s, u.y, py), qz = __fmaf_rn(s, u.z, pz);
    return dot3(qx, qy, qz, qx, qy, qz);
}

__global__ __launch_bounds__(MS_BLOCK) void k_ms_grid(const float4* rec, const long* tofs, long total_T, int n, float trunc, float* sdf) {
    __shared__ float4 tile[MS_TILE * MS_REC];
    const int m = blockIdx.y;
    const int npt = n * n * n;
    const int p = (int)(blockIdx.x * MS_BLOCK + threadIdx.x);
    const int pp = p < npt ? p : 0;                                 // (threads past the grid compute voxel 0 and store nothing)
    const float fn = (float)n;
    const float px = (float)(pp / (n * n)) / fn - 0.5f, py = (float)((pp / n) % n) / fn - 0.5f, pz = (float)(pp % n) / fn - 0.5f;
    const long t0 = clampl(tofs[m], 0, total_T), t1 = clampl(tofs[m + 1], t0, total_T);
    float best = INFINITY, wsum = 0.f;
    for (long base = t0; base < t1; base += MS_TILE) {
        const int cnt = (int)(t1 - base < MS_TILE ? t1 - base : MS_TILE);
        __syncthreads();
        for (int q = threadIdx.x; q < cnt * MS_REC; q += MS_BLOCK) tile[q] = rec[base * MS_REC + q];
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const float4* r = tile + t * MS_REC;
            const float4 r7 = r[7];
            if (__builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, r7.w)) != 0) continue;       // zero area (wave-uniform)
            const float4 A = r[0], B = r[1], C = r[2], Mab = r[3], Mbc = r[4], Mca = r[5], Uab = r[6], Uca = r[8];
            const float ax = A.x - px, ay = A.y - py, az = A.z - pz;
            const float bx = B.x - px, by = B.y - py, bz = B.z - pz;
            const float cx = C.x - px, cy = C.y - py, cz = C.z - pz;
            // the plane: h = a . n is minus the signed height of P; P projects into the triangle when it is on the inner side of all edges
            const float h = dot3(ax, ay, az, A.w, B.w, C.w);
            const float out = fmaxf(fmaxf(dot3(ax, ay, az, Mab.x, Mab.y, Mab.z), dot3(bx, by, bz, Mbc.x, Mbc.y, Mbc.z)),
                                    dot3(cx, cy, cz, Mca.x, Mca.y, Mca.z));
            const float e2 = fminf(fminf(seg_d2(ax, ay, az, Uab, Mab.w), seg_d2(bx, by, bz, r7, Mbc.w)), seg_d2(cx, cy, cz, Uca, Mca.w));
            best = fminf(best, out <= 0.f ? h * h : e2);
            // half the solid angle.  v_sqrt_f32 (1 ulp) for the three lengths: sqrtf is the correctly rounded root with its denormal
            // scaling, 17 instructions each and a quarter of the loop; an ulp on a length moves the angle by ~1e-7
            // (profiles/mesh_sdf_notes.md)
            const float la = es_ms_len(ax, ay, az), lb = es_ms_len(bx, by, bz), lc = es_ms_len(cx, cy, cz);
            float den = la * lb * lc;
            den = __fmaf_rn(dot3(ax, ay, az, bx, by, bz), lc, den);
            den = __fmaf_rn(dot3(bx, by, bz, cx, cy, cz), la, den);
            den = __fmaf_rn(dot3(cx, cy, cz, ax, ay, az), lb, den);
            wsum += atan2f(h * Uab.w, den);
        }
    }
    if (p < npt) {
        const float d = sqrtf(best);
        const float v = wsum * 0.15915494309189533577f > 0.5f ? -d : d;
        sdf[(long)m * npt + p] = fminf(fmaxf(v, -trunc), trunc);
    }
}

}  // namespace

extern "C" size_t es_mesh_sdf_workspace(int K, long total_T) {
    if (K <= 0 || total_T < 0) return 0;
    return (size_t)K * 4 * sizeof(double) + (size_t)total_T * MS_REC * sizeof(float4);       // frames, then records (16-byte aligned)
}

extern "C" int es_mesh_sdf(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* tri_offset, int K,
                           long total_V, long total_T, int n, float trunc, float fit, void* workspace, int32_t* bad_flags,
                           float* transform, float* sdf, es_stream stream) {
    ES_REQUIRE(verts && faces && vert_offset && tri_offset && workspace && bad_flags && sdf,
               "es_mesh_sdf: NULL pointer (verts %p faces %p vert_offset %p tri_offset %p workspace %p bad_flags %p sdf %p)", (const void*)verts,
               (const void*)faces, (const void*)vert_offset, (const void*)tri_offset, workspace, (void*)bad_flags, (void*)sdf);
    ES_REQUIRE(((uintptr_t)workspace & 15) == 0, "es_mesh_sdf: workspace must be 16-byte aligned");
    ES_REQUIRE(K > 0 && K <= 65535, "es_mesh_sdf: K = %d meshes (1 .. 65535)", K);
    ES_REQUIRE(n >= 2 && n <= 1290, "es_mesh_sdf: n = %d (2 .. 1290: n^3 must fit int32)", n);
    ES_REQUIRE((long)K * n * n * n <= 2147483647L, "es_mesh_sdf: K * n^3 = %ld is beyond int32 indexing", (long)K * n * n * n);
    ES_REQUIRE(total_V >= 0 && total_V <= 2147483647L, "es_mesh_sdf: total_V = %ld (0 .. 2^31 - 1)", total_V);
    ES_REQUIRE(total_T >= 0 && total_T <= 2147483647L / (3 * MS_REC), "es_mesh_sdf: total_T = %ld is beyond int32 indexing (0 .. %ld)",
               total_T, 2147483647L / (3 * MS_REC));
    ES_REQUIRE(trunc > 0.f && trunc < INFINITY, "es_mesh_sdf: trunc = %g (must be positive and finite)", (double)trunc);
    ES_REQUIRE(fit == fit && fit < INFINITY, "es_mesh_sdf: fit = %g (<= 0: no fit; else the longest side of the fitted box)", (double)fit);
    double* frame = (double*)workspace;
    float4* rec = (float4*)(frame + 4 * (long)K);
    const int npt = n * n * n;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ms_frame, dim3(K), dim3(MS_BLOCK), 0, s, verts, (const long*)vert_offset, total_V, fit, frame, transform, bad_flags);
    if (total_T > 0)
        hipLaunchKernelGGL(k_ms_prep, dim3((unsigned)((total_T + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, s, verts, faces,
                           (const long*)vert_offset, (const long*)tri_offset, K, total_V, total_T, (const double*)frame, rec, bad_flags);
    hipLaunchKernelGGL(k_ms_grid, dim3((npt + MS_BLOCK - 1) / MS_BLOCK, K), dim3(MS_BLOCK), 0, s, (const float4*)rec,
                       (const long*)tri_offset, total_T, n, trunc, sdf);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}
