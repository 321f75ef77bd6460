// The route of one es_conv_mfma_f16 launch: which kernel runs on which grid, where the fp32 K sum is cut and how many slabs land in
// the workspace.  Host arithmetic on the arguments and the route options only -- no HIP header, no hip* call: es_conv_route.hip also
// compiles as plain C++ (tests/c/conv_route_sweep.cpp links it under the host sanitizers).
// conv_route() DECIDES, conv_launch() (es_vol.hip) LAUNCHES what the route names and decides nothing, the planner's queries
// (es_conv_emits_gn_stats / _gn_part / es_conv_split_of / es_conv_kernel_of / es_conv_fold_balanced / es_conv_route_of) read fields.
// Shard bit-equality, the workspace's slab count and a model file's replay all rest on this rule: keep it in conv_route().
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/echoscene_hip.h"
#include "es_error.h"

constexpr int BN = 224;        // output columns of a workgroup tile (es_vol.hip: the implicit-GEMM kernels)
constexpr int GN_VT = 64;      // voxels per tile of the GroupNorm statistics pass, at most

struct ConvGeom {
    int O, D, H, W;          // output grid
    int Hi, Wi;              // input grid (H,W may differ from output for DOWN/UP)
    int Di;                  // input depth (differs from D for DOWN_DHW / UP_DHW)
    int lw, lh, ld;          // log2 of W, H, D (output)
};

// The kernel families; k_conv_ws has one value per tile built: rows, consumer waves, producer waves, ring depth
enum class ConvKernel {
    none,                      // nothing conv_launch() can launch: a chunked route, or forcing options that name a tile that is not built
    small_n, small_n_tiled, n16, kw_4_1, kw_2_2, ws_256_8_4_3, ws_64_4_4_3, ws_64_4_4_6, ws_128_4_4_3, ws_128_4_8_3, ws_128_4_8_5, ws3,
    ws_256_up_fold,            // k_conv_ws_fold: ws_256_8_4_3 of an UP_HW launch on its folded weight image (12 K units per chunk, not 27)
    linear_ws, linear_deep, lean_256, lean_128, lean_64
};
// the enumerators' spelling, in their order (es_conv_kernel_of; es_conv_route_info.kernel indexes it): a kernel added to the enum is added here
extern const char* const kConvKernelName[(int)ConvKernel::lean_64 + 1];
enum class ConvReduce { none, plain, gn_part };      // k_conv_splitk_reduce / k_conv_splitk_reduce_gn behind a launch split over workgroups

// Which rule cut K for this launch.  choose_split() tries them in THIS order and the first that applies sets S, once.
enum class SplitRule {
    direct,                    // small_n / small_n_tiled / n16 and chunked launches: no tile, nothing to cut here
    forced_tile,               // tools: conv_st_bm / conv_kw_ks put the launch on the tile they name, cut as the caller says
    few_plain,                 // few objects: a plain split over workgroups chosen for the REFERENCE problem (1: none, on small tiles)
    few_kstreams,              // few objects: 4 K streams -- inside the workgroup (k_conv_kw, S = 1) or, on other tiles, over workgroups
    caller,                    // the caller's explicit splitk > 0
    rows256,                   // small problem kept on 256-row tiles, K split until about one workgroup per CU runs
    deep,                      // k_linear_deep: K-short plain linear, one round of 64-row tiles, never split
    tiny,                      // tiny K-short problem: K split over 64-row tiles
    fill256,                   // enough 256-row tiles, but the last round of workgroups mostly empty: the smallest split that fills it
    auto128,                   // the automatic split of a small problem on 128-row tiles
    none                       // no rule applies (or splitk == 0): S = 1
};

struct ConvRoute {
    ConvGeom g;
    int ncdhw;
    long M;                    // rows of this launch
    long omax;                 // > 0: over the 2 GiB descriptor limit -- launched in chunks of omax objects, each with a route of its own
    ConvKernel kernel;
    unsigned gx = 1, gy = 1, gz = 1;      // the grid (conv_launch() builds the dim3)
    size_t lds;                // small_n / small_n_tiled: dynamic LDS bytes (the other kernels' are constants of their launchers)
    SplitRule rule;            // the rule that set S
    int S;                     // split of K over workgroups (gz; 1: none)
    int ncb;                   // linear_ws: column tiles a workgroup walks
    bool upm, geglu;
    char unbuilt[96];          // kernel == none behind forcing options: what conv_launch() reports
    bool epi_stats;            // the kernel's epilogue can form the row-group sums of gn_stats_out (es_conv_emits_gn_stats)
    bool stats;                // ... and does in this launch: gn_stats_out is given
    bool part_ok;              // the reduction can form a GroupNorm's per-tile partial sums (es_conv_emits_gn_part)
    ConvReduce reduce;
    int vt;                    // gn_part: voxel tile of the partial sums
    bool stats_pass;           // k_rowgroup_stats over the finished output forms gn_stats_out
    int slabs;                 // es_conv_split_of: fp32 slabs [slabs][M][N] written into the workspace (= S behind every tiled route; a chunked
                               // launch: in units of the whole M x N; 0: a direct kernel, no workspace)
    bool fold_bal;             // ws_256_up_fold on its balanced schedule (k_conv_ws_fold_bal, grid (row tiles, 2); es_conv_fold_balanced)
};

// ---- Route options of the volume path (no environment access for anything that changes bits) ------------------------------------
// Everything below decides WHERE an fp32 sum is cut (split-K factors, which kernel forms a GroupNorm's sums) or which kernel family
// multiplies: it changes the bits of the results.  Once these were process-environment switches read inside the library: two
// ranks -- or a process that saves a model file and one that replays it -- with different environments silently disagreed.  Now they
// are process-wide options with constant defaults that ONLY an explicit es_vol_set_option() call changes (tests and A/B tools);
// es_model_save records them in the file and es_model_load refuses a file written under other values.  conv_route() is the only
// reader of the conv_* options (gn_rg: gn_route(), the rule of es_groupnorm_vol).  The three env_* members are NOT options: environment switches -- ES_CONV_A3,
// ES_CONV_LINWS, ES_CONV_N16 -- that move a launch between kernels with the same K order and the same bits, read
// once per process and recorded nowhere; the A/B switches whose variant lost (ES_CONV_NS, ES_CONV_GB, ES_LIN_RING, ES_LIN_NCB_MAX)
// went with the kernel variants only they reached.
struct RouteOptions {
    int conv_tile = 0;             // 128: force 128-row tiles
    int conv_force256 = 0;         // 1: 256-row producer/consumer tiles for any problem size (tests)
    int conv_ws = 1;               // 0: k_conv_lean instead of the warp-specialised k_conv_ws
    int conv_wssplit = 1;          // 0: small problems on 128- / 64-row tiles instead of 256-row tiles with split K
    int conv_wss_target = 256;     // workgroup target of that split
    int conv_deep = 1;             // 0: no k_linear_deep for small K-short linear launches
    int conv_tinysplit = 1;        // 0: tiny K-short launches without split K
    int gn_rg = 1;                 // 0: GroupNorm statistics always from a pass over the tensor
    int conv_few = 1;              // 0: the few-objects routes off (the older routing for small problems)
    int conv_st_bm = 0;            // tools only: 64 / 128 = every producer/consumer-eligible launch on k_conv_ws tiles of that many rows
    int conv_st_np = 4;            // tools only: producer waves of that tile (4; 8 with 128-row tiles)
    int conv_st_ns = 3;            // tools only: ring depth of that tile (3; 6 with 64-row tiles, 5 with 128-row tiles and 8 producers)
    int conv_kw_ks = 0;            // tools only: 4 / 2 = every eligible launch on k_conv_kw with that many K streams per workgroup
    int env_a3 = 1;                // ES_CONV_A3 (unset: ES_CONV_A3_DEFAULT): k_conv_ws3 where it applies
    int env_linws = 1;             // ES_CONV_LINWS = 0: no k_linear_ws
    int env_n16 = 1;               // ES_CONV_N16 = 0: no k_conv_n16
};
// the process-wide instance: es_vol_set_option() writes it, es_vol_options() prints it, the extern "C" queries, es_conv_mfma_f16 and
// es_groupnorm_vol (gn_route(): gn_rg) read it
const RouteOptions& es_route_options();

// The pure function: 0 and the route in *r, or 2 with es_set_error() on arguments the conv refuses
int conv_route(const es_conv_args& a, const RouteOptions& o, ConvRoute* r);

// The arguments of one chunk of a launch over the 2 GiB descriptor limit: n objects from object o0 on -- O, the O_hint that keeps the
// split-K choice of the whole (or the reference) problem, the operand and output pointers advanced, no GroupNorm sums (the planes
// are laid out for the whole tensor: one pass behind the chunks; partials: never asked for).  g: the whole launch's geometry.
es_conv_args conv_chunk_args(const es_conv_args& a, const ConvGeom& g, long o0, long n);

// voxel-tile size of the GroupNorm statistics pass by workgroup count: small problems (few objects per GPU when sharded) get smaller
// tiles; Oh = the object count of the WHOLE problem (O_hint) so that a shard tiles like the unsharded run
inline int gn_voxel_tile(long Oh, int V) {
    int vt = GN_VT;
    while (vt > 8 && Oh * ((V + vt - 1) / vt) < 512) vt >>= 1;
    return vt;
}

// log2 of TX, the lanes k_gn_apply lays across the 8-channel chunks of a voxel: the chunk count rounded up to a power of two, at most
// 32 (constexpr: the kernel itself evaluates this rule, gn_route() reports it)
constexpr int gn_apply_log2_tx(int c8n) {
    int lt = 5;
    while (lt > 0 && (1 << (lt - 1)) >= c8n) --lt;
    return lt;
}

// ---- The route of one es_groupnorm_vol launch: gn_route() DECIDES (tiles, statistics source, whether k_gn_finalize runs, where the
// final statistics go, voxels per apply block, every grid), es_groupnorm_vol (es_vol.hip) LAUNCHES what it names and decides nothing,
// es_groupnorm_route_of reads it for tests.
enum class GnStats { pass = ES_GN_STATS_PASS, part_in = ES_GN_STATS_PART_IN, rowgroup = ES_GN_STATS_ROWGROUP };
struct GnRoute {
    int vt, ntiles;
    GnStats src;
    bool finalize;             // k_gn_finalize (long tile lists: the statistics reduced once per object, not in every apply block)
    long fin_off;              // floats from es_gn_args.stats to the final statistics k_gn_apply reads; -1: it reduces the partials itself
    int vpb, TX;
    unsigned partial_gx, partial_gy, fin_gx, fin_gy, apply_gx, apply_gy;      // 0, 0: that launch does not run
};
// 0 and the route in *r, or 2 with es_set_error() on arguments the GroupNorm refuses
int gn_route(const es_gn_args& a, const RouteOptions& o, GnRoute* r);

// ---- The instantiation of one es_attention_f16 / es_attention_f32 launch (es_attention_route_of reads it for tests)
enum class AttnKernel { h32_1, h32_2, h64_1, h64_2, h96_1, h96_2, h256_1, f32m_64, f32m_96, f32_64, f32_96 };
extern const char* const kAttnKernelName[(int)AttnKernel::f32_96 + 1];
struct AttnRoute {
    AttnKernel kernel;
    int DP, rows;              // padded head dimension, query rows per workgroup
    unsigned gx, gy;
    int block;                 // threads per workgroup
    size_t lds;                // dynamic LDS bytes
};
int attn_route(const es_attn_args& a, bool fp32, AttnRoute* r);
