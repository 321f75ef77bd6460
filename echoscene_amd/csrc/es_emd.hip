// Earth mover's distance between point clouds (the EMD half of the reference's
// scripts/compute_mmd_cov_1nn.py): out[i, j] = min over one-to-one matchings sigma of mean_p |a_ip - b_j,sigma(p)|, Euclidean, the value
// of the reference's emd_approx, which solves one assignment problem per pair on the host.  Here one workgroup solves one pair with
// an integer eps-scaling auction (Bertsekas 1988) in Jacobi rounds; tests/emd_ref.py restates it in numpy, step by step.
//
// Arithmetic
//   scale  m = the largest extent of the joint bounding box of the two clouds (fp32 subtraction), 2^(k-1) <= m < 2^k;
//          e = max(3, k + 1).  Every distance is below sqrt(3) m (1 + 2^-23) < 2^e.  Clouds normalised as the metric script leaves them
//          (|coordinate| <= 1) have e = 3; e > 62 (squares would overflow) is refused as status 2.
//   cost   c_ij = rint(d_ij * 2^(23 - e)), d_ij = sqrt((dx dx + dy dy) + dz dz) from direct fp32 differences, every operation rounded
//          once (no fma contraction, correctly rounded sqrt): an integer in [0, 2^23], exact in fp32, the same bits in numpy.
//   bid    an unassigned bidder i scans w_j = c_ij + price_j over all objects for the smallest (the lowest j among equals) and the
//          smallest of the others, and bids inc = w2 - w1 + eps >= eps on j1.  Per object the largest inc wins, the lowest bidder
//          among equals: one LDS atomic max on the key (inc << 16 | 0xffff - i), an integer maximum, so the order in which the waves
//          arrive does not matter.  The winner replaces the owner, who becomes unassigned; price_j1 += inc.
//   phases eps = max(1, cmax / 2), then max(1, eps / 5) ... down to 1 (cmax = the largest c_ij of the pair).  Prices carry over, the
//          assignment starts empty.  P = 1 has no second object and is assigned directly.
//   value  sum_j c(owner_j, j) (an integer sum: any order) * 2^(e - 23) / P in double, rounded to fp32 once.
// All bidders of a round see the prices of its start (Jacobi), ties are broken by index, and nothing else enters: an entry's bits
// depend on its two clouds and their order alone.
//
// EMD_EPS = 4e-6 at e = 3, 4e-6 * 2^(e - 3) in general; with u = 2^-24 and q = 2^(e - 23) the quantum of a cost (2^-20 at e = 3):
//   distance   dx carries u, its square 3u, the two sums 5u, the root 2.5u + u: |fl(d) - d| <= 3.5 u d < 3.5 u 2^e      = 1.67e-6
//   quantum    |c q - fl(d)| <= q / 2                                                                                   = 0.48e-6
//   auction    at the end every bidder holds an object within eps = 1 of its best at the final prices (eps-complementary
//              slackness), so the assignment costs at most P * 1 more than the optimum of the integer costs: q per point  = 0.95e-6
//   mean       one fp32 rounding of a value < 2^e: u 2^e (the double product and quotient are below 2^-52 relative)       = 0.48e-6
//   A change of every cost by at most h moves the optimum by at most h, so opt - 2.15e-6 <= out <= opt + 3.58e-6 < EMD_EPS.
//
// Termination.  A bid raises a price by inc >= eps >= 1, so every round raises at least one price by at least eps.  Prices are
// bounded: a bid sets price_j = w2 - c_ij + eps <= price_k + cmax + eps for every other object k.  While the phase lasts an object u
// is still unassigned and keeps its price from the phase's start, at most M0, the largest price then; so price_j <= M0 + cmax + eps
// unless j = u is the last one, whose bid ends the phase at <= M0 + 2 (cmax + eps).  Over all phases: price < 2 phases (cmax + eps_0)
// <= 2 * 11 * 1.5 * 2^23 = 2.8e8 < 2^31 (int32 prices and sums cannot overflow), and a phase has at most P * that / eps rounds: the
// loop ends.  That proven bound (1e12 rounds at P = 5000) is no guard for a shared machine, so the loop also carries a hard cap:
// EM_CAP_MULT * P + EM_CAP_ADD = 128 P + 4096 rounds per phase and EM_CAP_TOTAL_MULT * P + EM_CAP_ADD = 512 P + 4096 over all phases
// (fewer where the scaled cost range cmax gives so few phases that phases * the first is less).  Origin: rounds per phase measured
// with the restatement -- at most 1.9 P on the test clouds up to P = 1025, 6.0 P on the worst of the adversarial ones (every point of
// one cloud coincident: all bidders want the same objects), 8.3 P on clouds of 2048 points -- and rounds over all phases: 38 P on
// that adversarial pair and, on the GPU, at most 36 P among 16384 pairs of 2048 points and 33 P among 256 pairs of 5000
// (profiles/emd_notes.md).  The caps are 15 times the largest phase and 13 times the largest total seen.  Why they are not reached
// by valid input is therefore an observation with that margin, not a theorem: the proof above gives termination, not a useful count.
// What a pair can cost at the very most: 512 P + 4096 rounds at the 9 us (P = 2048) to 19 us (P = 5000) measured per round, that
// is 10 s at 2048 points and 50 s at EM_MAX_POINTS = 5120.  A pair that reaches a cap stops, returns NaN and status 1, and the
// wrapper raises.
//
// Layout.  EM_BLOCK = 1024 threads, 16 waves; a wave takes one bidder at a time and its 64 lanes scan the objects (consecutive
// floats of the staged cloud b: no bank conflict), then merge (w1, j1, w2) over the lanes.  Dynamic LDS, 29 bytes per point:
// key 8, b 12 (x, y, z planes), price 4, list of unassigned bidders 2, owner 2, assigned flag 1 -- 145 KB at P = 5000, one
// workgroup per CU; 59 KB at 2048, two.  Two is also the most at any smaller P: the kernel takes 64 VGPRs, 8 waves per SIMD, 32
// waves per CU, which is two workgroups of 16 waves (and the 2048 threads of a CU).  A matrix of small clouds therefore runs two
// pairs per CU with most of their waves idle; a smaller workgroup for small P is a follow-up.  EM_MAX_POINTS = 5120.  A round is
// three barriers: bids | resolve per object | rebuild the list.  The bidder's coordinates come from global memory, loaded one
// bidder ahead.
#include "es_common.h"
#include <mutex>

#pragma clang fp contract(off)

namespace {

constexpr int EM_BLOCK = 1024;
constexpr int EM_WAVES = EM_BLOCK / 64;
constexpr int EM_MAX_POINTS = 5120;
constexpr int EM_COST_BITS = 23;
constexpr int EM_MIN_EXP = 3, EM_MAX_EXP = 62;
constexpr int EM_THETA = 5;
constexpr int EM_CAP_MULT = 128, EM_CAP_ADD = 4096;      // rounds per phase: EM_CAP_MULT * P + EM_CAP_ADD
constexpr int EM_CAP_TOTAL_MULT = 512;                   // rounds over all phases: EM_CAP_TOTAL_MULT * P + EM_CAP_ADD
constexpr int EM_TAIL = 512;                    // bytes after the arrays: counters (32) and the wave partials of the bounding box (384)
constexpr int EM_BIG = 0x7fffffff;

__host__ __device__ constexpr int em_pad(int P) { return (P + 7) & ~7; }
__host__ __device__ constexpr size_t em_lds_bytes(int P) { return (size_t)29 * em_pad(P) + EM_TAIL; }
static_assert(em_lds_bytes(EM_MAX_POINTS) <= 160 * 1024, "the cloud state of EM_MAX_POINTS points must fit the LDS of a CU");
static_assert(32 + EM_WAVES * 3 * 2 * 4 <= EM_TAIL, "counters and bounding-box partials must fit the tail");
static_assert(EM_MAX_POINTS < 32768, "a bidder index takes 16 bits of the bid key and 15 of an owner entry");

// the scaled integer cost of (x, y); every operation rounded once, as numpy does: plain operators with contraction switched off for
// this file (the __fmul_rn family inlines to operators that carry the header's own contract flag and fuse), sqrtf correctly rounded
__device__ __forceinline__ int em_cost(float x0, float x1, float x2, float y0, float y1, float y2, float scale) {
    const float dx = x0 - y0, dy = x1 - y1, dz = x2 - y2;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float d2 = (xx + yy) + zz;
    return (int)rintf(__builtin_sqrtf(d2) * scale);
}

// 8 waves per SIMD = two workgroups per CU, which needs at most 64 VGPRs: the scan loops are kept rolled (unrolled by 8 the compiler
// took 104, one workgroup per CU, whatever the LDS left free)
__global__ __launch_bounds__(EM_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_emd_matrix(const float* a, const float* b, int Nb, int P, int symmetric, float* out,
                                                        int32_t* status, int32_t* rounds_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = (int)(blockIdx.x / (unsigned)Nb), j = (int)(blockIdx.x % (unsigned)Nb);
    const long o_ij = (long)i * Nb + j, o_ji = (long)j * Nb + i;
    if (symmetric) {                                                // pairs with i < j, mirrored; the diagonal is exactly 0
        if (i > j) return;
        if (i == j) {
            if (tid == 0) {
                out[o_ij] = 0.f;
                status[o_ij] = 0;
                if (rounds_out) rounds_out[o_ij] = 0;
            }
            return;
        }
    }
    const int Pp = em_pad(P);
    unsigned long long* key = (unsigned long long*)smem;            // [Pp] the best bid of the round per object, 0: none
    float* bx = (float*)(smem + (size_t)8 * Pp);                    // [3][Pp] the objects
    float* by = bx + Pp;
    float* bz = by + Pp;
    int* price = (int*)(bz + Pp);                                   // [Pp]
    unsigned short* list = (unsigned short*)(price + Pp);           // [Pp] the unassigned bidders of the round
    short* owner = (short*)(list + Pp);                             // [Pp] bidder per object, -1: none
    unsigned char* has = (unsigned char*)(owner + Pp);              // [Pp] bidder holds an object
    char* tail = smem + (size_t)29 * Pp;
    unsigned long long* total = (unsigned long long*)tail;          // [1]
    int* cnt = (int*)(tail + 8);                                    // [1] length of the list being rebuilt
    int* cmax_s = (int*)(tail + 12);                                // [1]
    int* bad_s = (int*)(tail + 16);                                 // [1]
    float* box = (float*)(tail + 32);                               // [EM_WAVES][3][2]: min and max per wave and axis

    const float* ai = a + (long)i * P * 3;
    const float* bj = b + (long)j * P * 3;

    // stage b, clear the state, look at every coordinate: finite? the joint bounding box
    if (tid == 0) {
        *total = 0ull;
        *cnt = 0;
        *cmax_s = 0;
        *bad_s = 0;
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int p = tid; p < P; p += EM_BLOCK) {
        const float y0 = bj[3 * p], y1 = bj[3 * p + 1], y2 = bj[3 * p + 2];
        const float x0 = ai[3 * p], x1 = ai[3 * p + 1], x2 = ai[3 * p + 2];
        bx[p] = y0;
        by[p] = y1;
        bz[p] = y2;
        price[p] = 0;
        key[p] = 0ull;
        bad |= !(isfinite(y0) && isfinite(y1) && isfinite(y2) && isfinite(x0) && isfinite(x1) && isfinite(x2));
        lo[0] = fminf(lo[0], fminf(x0, y0));
        lo[1] = fminf(lo[1], fminf(x1, y1));
        lo[2] = fminf(lo[2], fminf(x2, y2));
        hi[0] = fmaxf(hi[0], fmaxf(x0, y0));
        hi[1] = fmaxf(hi[1], fmaxf(x1, y1));
        hi[2] = fmaxf(hi[2], fmaxf(x2, y2));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], w));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], w));
        }
    __syncthreads();                                                // (the counters are cleared)
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            box[(wave * 3 + c) * 2] = lo[c];
            box[(wave * 3 + c) * 2 + 1] = hi[c];
        }
    }
    if (bad) atomicOr(bad_s, 1);
    __syncthreads();
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float l = INFINITY, h = -INFINITY;
        for (int w = 0; w < EM_WAVES; ++w) {
            l = fminf(l, box[(w * 3 + c) * 2]);
            h = fmaxf(h, box[(w * 3 + c) * 2 + 1]);
        }
        m = fmaxf(m, h - l);
    }
    const int e = max(EM_MIN_EXP, (int)((__float_as_uint(m) >> 23) & 0xff) - 126 + 1);
    if (*bad_s || !isfinite(m) || e > EM_MAX_EXP) {                 // (uniform) flagged, never iterated on
        if (tid == 0) {
            out[o_ij] = NAN;
            status[o_ij] = 2;
            if (rounds_out) rounds_out[o_ij] = 0;
            if (symmetric) {
                out[o_ji] = NAN;
                status[o_ji] = 2;
                if (rounds_out) rounds_out[o_ji] = 0;
            }
        }
        return;
    }
    const float scale = __uint_as_float((unsigned)(127 + EM_COST_BITS - e) << 23);      // 2^(23 - e), a normal number for e <= 62

    int rounds = 0, capped = 0;
    if (P == 1) {
        if (tid == 0) owner[0] = 0;
    } else {
        // the largest cost of the pair
        int cm = 0;
        for (int t = wave; t < P; t += EM_WAVES) {
            const float x0 = ai[3 * t], x1 = ai[3 * t + 1], x2 = ai[3 * t + 2];
#pragma unroll 1
            for (int q = lane; q < P; q += 64) cm = max(cm, em_cost(x0, x1, x2, bx[q], by[q], bz[q], scale));
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) cm = max(cm, __shfl_xor(cm, w));
        if (lane == 0) atomicMax(cmax_s, cm);
        __syncthreads();
        const int cmax = *cmax_s;
        const int cap_phase = EM_CAP_MULT * P + EM_CAP_ADD, cap_total = EM_CAP_TOTAL_MULT * P + EM_CAP_ADD;      // (<= 512 * 5120 + 4096)

        for (int eps = max(1, cmax / 2);; eps = max(1, eps / EM_THETA)) {
            for (int p = tid; p < P; p += EM_BLOCK) {
                owner[p] = (short)-1;
                has[p] = 0;
                list[p] = (unsigned short)p;
            }
            __syncthreads();
            int n_un = P, phase_rounds = 0;
            while (n_un > 0) {
                if (phase_rounds == cap_phase || rounds + phase_rounds == cap_total) {
                    capped = 1;
                    break;
                }
                // bids: one bidder per wave at a time, its coordinates loaded one bidder ahead
                int t = wave;
                float x0 = 0.f, x1 = 0.f, x2 = 0.f;
                if (t < n_un) {
                    const int bi = list[t];
                    x0 = ai[3 * bi], x1 = ai[3 * bi + 1], x2 = ai[3 * bi + 2];
                }
                while (t < n_un) {
                    const int bi = list[t];
                    const int tn = t + EM_WAVES;
                    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
                    if (tn < n_un) {
                        const int bn = list[tn];
                        n0 = ai[3 * bn], n1 = ai[3 * bn + 1], n2 = ai[3 * bn + 2];
                    }
                    int w1 = EM_BIG, w2 = EM_BIG, j1 = EM_BIG;
#pragma unroll 1
                    for (int q = lane; q < P; q += 64) {
                        const int w = em_cost(x0, x1, x2, bx[q], by[q], bz[q], scale) + price[q];
                        if (w < w1) {                               // (q rises: the lowest index among equals stays)
                            w2 = w1;
                            w1 = w;
                            j1 = q;
                        } else if (w < w2) w2 = w;
                    }
#pragma unroll
                    for (int s = 32; s > 0; s >>= 1) {
                        const int ow1 = __shfl_xor(w1, s), ow2 = __shfl_xor(w2, s), oj1 = __shfl_xor(j1, s);
                        if (ow1 < w1 || (ow1 == w1 && oj1 < j1)) {
                            w2 = min(w1, ow2);
                            w1 = ow1;
                            j1 = oj1;
                        } else w2 = min(w2, ow1);
                    }
                    if (lane == 0)                                  // P >= 2: j1 < P and w2 is a real value
                        atomicMax(&key[j1], ((unsigned long long)(unsigned)(w2 - w1 + eps) << 16) | (unsigned long long)(0xffff - bi));
                    t = tn;
                    x0 = n0, x1 = n1, x2 = n2;
                }
                __syncthreads();
                if (tid == 0) *cnt = 0;
                // per object: the winner replaces the owner (who did not bid: no two threads write one entry)
                for (int q = tid; q < P; q += EM_BLOCK) {
                    const unsigned long long k = key[q];
                    if (k) {
                        const int win = 0xffff - (int)(k & 0xffffull);
                        const int old = owner[q];
                        if (old >= 0) has[old] = 0;
                        owner[q] = (short)win;
                        has[win] = 1;
                        price[q] += (int)(k >> 16);
                        key[q] = 0ull;
                    }
                }
                __syncthreads();
                for (int p = tid; p < P; p += EM_BLOCK)
                    if (!has[p]) list[atomicAdd(cnt, 1)] = (unsigned short)p;       // (at most P entries; their order changes no result)
                __syncthreads();
                n_un = *cnt;
                ++phase_rounds;
            }
            rounds += phase_rounds;
            if (capped || eps == 1) break;
        }
    }
    __syncthreads();
    if (!capped) {
        unsigned long long part = 0ull;
        for (int q = tid; q < P; q += EM_BLOCK) {
            const int bi = owner[q];
            part += (unsigned long long)em_cost(ai[3 * bi], ai[3 * bi + 1], ai[3 * bi + 2], bx[q], by[q], bz[q], scale);
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) part += __shfl_xor(part, w);
        if (lane == 0) atomicAdd(total, part);
        __syncthreads();
    }
    if (tid == 0) {
        const float v = capped ? NAN : (float)((double)*total * ldexp(1.0, e - EM_COST_BITS) / (double)P);
        out[o_ij] = v;
        status[o_ij] = capped;
        if (rounds_out) rounds_out[o_ij] = rounds;
        if (symmetric) {
            out[o_ji] = v;
            status[o_ji] = capped;
            if (rounds_out) rounds_out[o_ji] = rounds;
        }
    }
}

}  // namespace

extern "C" int es_emd_max_points(void) { return EM_MAX_POINTS; }

extern "C" int es_emd_matrix_rounds(const float* a, int Na, const float* b, int Nb, int P, int symmetric, float* out, int32_t* status,
                                    int32_t* rounds, es_stream stream) {
    ES_REQUIRE(a && b && out && status, "es_emd_matrix: NULL pointer (a %p b %p out %p status %p)", (const void*)a, (const void*)b,
               (void*)out, (void*)status);
    ES_REQUIRE(Na > 0 && Nb > 0 && P > 0, "es_emd_matrix: empty clouds (Na=%d Nb=%d P=%d)", Na, Nb, P);
    ES_REQUIRE(P <= EM_MAX_POINTS, "es_emd_matrix: P = %d points per cloud, at most %d (the state of a pair lives in the LDS of one CU)", P,
               EM_MAX_POINTS);
    ES_REQUIRE((long)Na * P * 3 <= 2147483647L && (long)Nb * P * 3 <= 2147483647L,
               "es_emd_matrix: %d x %d x 3 or %d x %d x 3 coordinates are beyond int32 indexing", Na, P, Nb, P);
    ES_REQUIRE((long)Na * Nb <= 2147483647L, "es_emd_matrix: %d x %d pairs are beyond int32 indexing", Na, Nb);
    ES_REQUIRE(!symmetric || (b == a && Nb == Na), "es_emd_matrix: symmetric needs b == a with the same count (a %p [%d, %d, 3], b %p [%d, %d, 3])",
               (const void*)a, Na, P, (const void*)b, Nb, P);
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)k_emd_matrix, hipFuncAttributeMaxDynamicSharedMemorySize, (int)em_lds_bytes(EM_MAX_POINTS));
    });
    ES_REQUIRE(attr_err == hipSuccess, "es_emd_matrix: hipFuncSetAttribute failed: %s", hipGetErrorString(attr_err));
    hipLaunchKernelGGL(k_emd_matrix, dim3((unsigned)(Na * Nb)), dim3(EM_BLOCK), em_lds_bytes(P), (hipStream_t)stream, a, b, Nb, P,
                       symmetric ? 1 : 0, out, status, rounds);
    ES_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int es_emd_matrix(const float* a, int Na, const float* b, int Nb, int P, int symmetric, float* out, int32_t* status,
                             es_stream stream) {
    return es_emd_matrix_rounds(a, Na, b, Nb, P, symmetric, out, status, nullptr, stream);
}
