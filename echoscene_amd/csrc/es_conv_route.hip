// conv_route(): the routing rule of es_conv_mfma_f16 (es_conv_route.h), its options and the host-only queries that read it.
// Plain C++ in a .hip file (the library's build derives object names from the extension): no HIP header, no hip* call, no kernel.
#include "es_conv_route.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

const char* const kConvKernelName[] = {
    "none",
    "small_n", "small_n_tiled", "n16", "kw_4_1", "kw_2_2", "ws_256_8_4_3", "ws_64_4_4_3", "ws_64_4_4_6", "ws_128_4_4_3", "ws_128_4_8_3", "ws_128_4_8_5", "ws3",
    "ws_256_up_fold", "linear_ws", "linear_deep", "lean_256", "lean_128", "lean_64"
};

// ---- the options: one table of names, in the order es_vol_options() prints and model files record ------------------------------
#ifndef ES_CONV_A3_DEFAULT
#define ES_CONV_A3_DEFAULT true
#endif
namespace {
const struct { const char* name; int RouteOptions::*field; } kOptions[] = {
    {"conv_tile", &RouteOptions::conv_tile}, {"conv_force256", &RouteOptions::conv_force256}, {"conv_ws", &RouteOptions::conv_ws},
    {"conv_wssplit", &RouteOptions::conv_wssplit}, {"conv_wss_target", &RouteOptions::conv_wss_target}, {"conv_deep", &RouteOptions::conv_deep},
    {"conv_tinysplit", &RouteOptions::conv_tinysplit}, {"gn_rg", &RouteOptions::gn_rg}, {"conv_few", &RouteOptions::conv_few},
    {"conv_st_bm", &RouteOptions::conv_st_bm}, {"conv_st_np", &RouteOptions::conv_st_np}, {"conv_st_ns", &RouteOptions::conv_st_ns},
    {"conv_kw_ks", &RouteOptions::conv_kw_ks},
};

// the defaults and, read here once per process and nowhere else, the three timing-only environment switches (same K order, same bits)
RouteOptions& process_options() {
    static RouteOptions o = [] {
        RouteOptions v;
        const char* a3 = getenv("ES_CONV_A3");
        const char* lin = getenv("ES_CONV_LINWS");
        const char* n16 = getenv("ES_CONV_N16");
        v.env_a3 = a3 ? atoi(a3) != 0 : ES_CONV_A3_DEFAULT;
        v.env_linws = !(lin && atoi(lin) == 0);
        v.env_n16 = !(n16 && atoi(n16) == 0);
        return v;
    }();
    return o;
}
}  // namespace

const RouteOptions& es_route_options() { return process_options(); }

extern "C" int es_vol_set_option(const char* name, int value) {
    ES_REQUIRE(name != nullptr, "es_vol_set_option: null name");
    for (const auto& k : kOptions) if (!strcmp(k.name, name)) { process_options().*k.field = value; return 0; }
    ES_REQUIRE(false, "es_vol_set_option: unknown option '%s'", name);
}
// "name=value;name=value;..." of every route option, in a fixed order (what es_model_save records); returns the length needed
extern "C" int es_vol_options(char* out, int cap) {
    std::string s;
    for (const auto& k : kOptions) { s += k.name; s += '='; s += std::to_string(process_options().*k.field); s += ';'; }
    if (out && cap > 0) { strncpy(out, s.c_str(), (size_t)cap - 1); out[cap - 1] = 0; }
    return (int)s.size() + 1;
}

namespace {

int ilog2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}

// ---- step 1: what every route needs ---------------------------------------------------------------------------------------------
int route_geometry(const es_conv_args& a, ConvRoute* r) {
    ES_REQUIRE(a.Cin % 32 == 0 && a.Cin > 0, "es_conv_mfma_f16: Cin=%d must be a positive multiple of 32", a.Cin);
    ES_REQUIRE(a.taps == 27 || a.taps == 1, "es_conv_mfma_f16: taps=%d", a.taps);
    ES_REQUIRE(!a.a2 || (a.Cin2 % 32 == 0 && a.Cin2 > 0), "es_conv_mfma_f16: Cin2=%d", a.Cin2);
    ES_REQUIRE(a.out_f32 || a.out_f16, "es_conv_mfma_f16: no output");
    ES_REQUIRE(a.epilogue == ES_EPI_NONE || (a.epilogue == ES_EPI_GEGLU && a.N % 224 == 0 && a.out_f16 && !a.out_f32 && !a.res &&
                                             !a.rowvec && !a.a2 && a.bias && a.out_ld >= a.N / 2 && a.out_ld % 8 == 0 && a.splitk <= 1),
               "es_conv_mfma_f16: GEGLU epilogue needs N %% 224 == 0 (N=%d), bias, f16 output only, no split-K", a.N);
    ConvGeom& g = r->g;
    g.O = a.O; g.D = a.D; g.H = a.H; g.W = a.W;
    g.Hi = a.H; g.Wi = a.W;
    g.Di = a.D;
    if (a.mode == ES_CONV_DOWN_HW) { g.Hi = 2 * a.H; g.Wi = 2 * a.W; }
    ES_REQUIRE(a.mode >= ES_CONV_SAME && a.mode <= ES_CONV_DOWN_DHW_P01, "es_conv_mfma_f16: unknown mode %d", a.mode);
    if (a.mode == ES_CONV_DOWN_DHW || a.mode == ES_CONV_DOWN_DHW_P01) { g.Hi = 2 * a.H; g.Wi = 2 * a.W; g.Di = 2 * a.D; }
    if (a.mode == ES_CONV_UP_DHW) g.Di = a.D / 2;
    if (a.mode == ES_CONV_UP_HW || a.mode == ES_CONV_UP_DHW) { g.Hi = a.H / 2; g.Wi = a.W / 2; }
    g.lw = ilog2_exact(a.W); g.lh = ilog2_exact(a.H); g.ld = ilog2_exact(a.D);
    ES_REQUIRE(g.lw >= 0 && g.lh >= 0 && g.ld >= 0, "es_conv_mfma_f16: D,H,W must be powers of two (%d,%d,%d)", a.D, a.H, a.W);
    r->ncdhw = a.out_ld < 0 ? 1 : 0;                               // out_ld < 0 selects NCDHW fp32 output [O,N,V]
    ES_REQUIRE(!r->ncdhw || (a.out_f32 && !a.res && !a.out_f16), "es_conv_mfma_f16: NCDHW output is fp32-only, no residual");
    r->M = (long)a.O * a.D * a.H * a.W;
    return 0;
}

// ---- step 2: object chunks ------------------------------------------------------------------------------------------------------
// input bytes of one object: the first operand on the input grid, the fused skip's on the output grid
long obj_bytes_in(const es_conv_args& a, const ConvGeom& g) { return (long)g.Di * g.Hi * g.Wi * a.Cin * 2; }
long obj_bytes_in2(const es_conv_args& a) { return a.a2 ? (long)a.D * a.H * a.W * a.Cin2 * 2 : 0; }

// The kernels address their operands with 31-bit byte offsets from a buffer descriptor.  Larger tensors are processed in
// object chunks (every object is independent; O_hint keeps the split-K choice of the whole problem).
int route_chunks(const es_conv_args& a, const RouteOptions& o, ConvRoute* r) {
    const ConvGeom& g = r->g;
    const long per_obj_in = obj_bytes_in(a, g), per_obj_in2 = obj_bytes_in2(a);
    const long halo = 4L * ((g.Hi + 1) * g.Wi + 1) * a.Cin;
    const long lim = (1L << 31) - halo - 1;
    long omax = a.O;
    if (per_obj_in > 0) omax = std::min(omax, lim / per_obj_in);
    if (per_obj_in2 > 0) omax = std::min(omax, lim / per_obj_in2);
    ES_REQUIRE(omax >= 1, "es_conv_mfma_f16: one object exceeds 2 GiB of input (%ld bytes)", per_obj_in);
    if (omax >= a.O) return 0;
    // a chunked launch forms no GroupNorm sums in its epilogues; its chunks split K as launches of omax objects do (with
    // O_hint: as the whole / the reference problem does) and write their slabs into the SAME workspace: report the slab
    // count in units of the whole launch's M x N (es_conv_split_of: the planner sizes the workspace with it)
    ConvRoute rc;
    if (int err = conv_route(conv_chunk_args(a, g, 0, omax), o, &rc)) return err;
    r->omax = omax;
    r->S = rc.S;                                                   // (es_conv_kernel_of: the split of a full chunk)
    r->slabs = (int)((rc.slabs * omax + a.O - 1) / a.O);
    r->stats_pass = a.gn_stats_out != nullptr;                     // (the planes are laid out for the whole tensor: one pass behind the chunks)
    return 0;
}

// ---- step 3: the two direct kernels ---------------------------------------------------------------------------------------------
bool route_direct(const es_conv_args& a, const RouteOptions& o, ConvRoute* r) {
    // N <= 4 with a narrow input (VQ-VAE conv_out 64 -> 1 at 64^3): direct kernel, weights in the rows layout.  Wider
    // inputs (UNet eps conv 224 -> 3) go through the MFMA tile: 98 % column padding, but the direct kernel's 756
    // dependent 16-B loads per voxel cost 2.4x (O=32) to 10x (O=4) more than the padded tile.
    if (a.N <= 4 && a.taps == 27 && a.Cin <= 64) {
        const size_t lds_t = (size_t)1000 * (a.Cin * 2 + 16) + (size_t)a.N * 27 * a.Cin * 2;
        const bool tiled = a.D % 8 == 0 && a.H % 8 == 0 && a.W % 8 == 0 && a.Cin % 8 == 0 && lds_t <= 160 * 1024;
        r->kernel = tiled ? ConvKernel::small_n_tiled : ConvKernel::small_n;
        r->gx = (unsigned)(tiled ? (long)a.O * (a.D / 8) * (a.H / 8) * (a.W / 8) : (r->M + 255) / 256);
        r->lds = tiled ? lds_t : (size_t)a.N * 27 * a.Cin * 2;
        r->S = 1;
        return true;
    }
    // N <= 16 from a wide input, NCDHW fp32 output, no fusions (the UNet's output conv): halo'd LDS image + one MFMA column
    // (ES_CONV_N16: A/B switch, timing only: same K order, same bits; 0 = off)
    if (a.N <= 16 && a.taps == 27 && a.Cin > 64 && r->ncdhw && a.mode == ES_CONV_SAME && !a.a2 && !a.res && !a.rowvec &&
        !a.out_f16 && a.D % 4 == 0 && a.H % 4 == 0 && a.W % 16 == 0 && o.env_n16 &&
        (long)a.O * a.D * a.H * a.W * a.Cin * 2 < (1L << 31)) {
        r->kernel = ConvKernel::n16;
        r->gx = (unsigned)((long)a.O * (a.D / 4) * (a.H / 4) * (a.W / 16));
        r->S = 1;
        return true;
    }
    return false;
}

// ---- step 4: the sizes the tiled routes are chosen by ---------------------------------------------------------------------------
// Tile / split choice by workgroup count (256 CUs x 2 resident workgroups):
//   >= 256 workgroups of 256 rows -> 8-wave 256x224 tiles;
//   otherwise 128x224 tiles, and when even those give < 512 workgroups (16x4x4 level: M = 8192) K is split
//   over S workgroups per tile (fixed-order reduction kernel, deterministic).
// small-M layers (16x4x4 level): 64-row tiles double the number of workgroups (>= 1 per CU)
struct TileCounts {
    long t256, t128, t64;      // tiles of 256 / 128 / 64 rows x 224 columns
    long t64h;                 // tiles of 64 rows x 112 columns (k_conv_kw's column halves)
};
TileCounts tile_counts(long rows, int N) {
    const long ntn = (N + BN - 1) / BN;
    return {((rows + 255) / 256) * ntn, ((rows + 127) / 128) * ntn, ((rows + 63) / 64) * ntn, ((rows + 63) / 64) * ((N + 111) / 112)};
}
// THIS launch: what picks the tile that realises a split
struct LaunchSize {
    long M;
    int ntn, nks;              // column tiles; K units of 32 channels x one tap, the fused skip's included
    TileCounts wg;
    bool can_split;            // a workspace, and an output the reduction kernels can write
    bool ws;                   // the producer/consumer kernels take it
    int forced_ks, forced_bm;  // tools: K streams of k_conv_kw / rows of the k_conv_ws tile every eligible launch is put on (0: none)
};
// The REFERENCE problem, which alone decides where K is cut: the WHOLE problem when this launch is one shard of it (O_hint > O), and with
// O_hint < 0 the CANONICAL arithmetic of a reference shard of -O_hint objects, whatever the launch's own object count -- every rank of
// every world size (1 included) cuts K where a shard of that size is cut best, so all of them leave the same bits and the small shards
// are the fast ones (once the reference was the unsharded run and its shards paid 2x)
struct RefSize {
    long Oh;
    TileCounts hg;
    int slab_cap;              // workspace contract (echoscene_hip.h): 16 slabs for small outputs, else 8
    bool small;                // fewer than 256 tiles of 256 rows, and no option that pins the tile: the few-objects regime
};
long ref_objects(const es_conv_args& a) { return a.O_hint < 0 ? -(long)a.O_hint : (long)(a.O_hint > a.O ? a.O_hint : a.O); }

LaunchSize launch_size(const es_conv_args& a, const RouteOptions& o, const ConvRoute& r) {
    LaunchSize L;
    L.M = r.M;
    L.ntn = (a.N + BN - 1) / BN;
    L.nks = a.taps * (a.Cin / 32) + (a.a2 ? a.Cin2 / 32 : 0);
    L.wg = tile_counts(r.M, a.N);
    const bool vec_out = !r.ncdhw && a.N % 4 == 0 && a.out_ld % 4 == 0 && (!a.rowvec || a.rowvec_ld % 4 == 0);
    L.can_split = a.workspace && vec_out;
    // k_conv_ws's epilogue is compiled for vector-aligned channels-last outputs addressed with 32-bit element offsets
    L.ws = o.conv_ws != 0 && vec_out && r.M * (long)a.out_ld < (1L << 30) && r.M * (long)a.N < (1L << 30) &&
           (!a.rowvec || (a.D * a.H * a.W) % 64 == 0);             // a wave's 64 rows in one object: rowvec per wave
    // tools: every eligible launch on the small producer/consumer tiles
    L.forced_ks = L.ws && (!r.geglu || !r.upm) ? o.conv_kw_ks : 0;
    L.forced_bm = L.forced_ks ? 64 : (L.ws && (!r.geglu || !r.upm) ? o.conv_st_bm : 0);
    return L;
}
RefSize ref_size(const es_conv_args& a, const RouteOptions& o) {
    RefSize R;
    R.Oh = ref_objects(a);
    const long Mh = R.Oh * a.D * a.H * a.W;
    R.hg = tile_counts(Mh, a.N);
    R.slab_cap = Mh * (long)a.N <= (1L << 22) ? 16 : 8;
    R.small = R.hg.t256 < 256 && o.conv_tile != 128 && o.conv_force256 != 1;
    return R;
}

// ---- step 5: the split rules.  Each answers its S (>= 1), or 0: "not my launch" -------------------------------------------------
int keep_units(int s, int nks, int units) {                        // the largest split <= s that leaves every part `units` K units
    while (s > 1 && nks / s < units) --s;
    return s;
}
int caller_split(const es_conv_args& a, const LaunchSize& L) { return a.splitk > 1 && L.can_split && a.epilogue != ES_EPI_GEGLU ? a.splitk : 1; }

// tools: split K as the caller says, 1 when it says nothing
int split_forced_tile(const es_conv_args& a, const RouteOptions&, const LaunchSize& L, const RefSize&) { return L.forced_bm ? caller_split(a, L) : 0; }

// The few-objects routes (fewer than 256 tiles of 256 rows in the reference problem).  What the REFERENCE problem decides -- a plain
// split of S over workgroups, or S = 4 K streams inside the workgroup (k_conv_kw, no slabs; the same bits as a plain split of 4).
// The launch's own row count only picks the tile that realises that split (few_tile_rows): 64- / 128-row producer/consumer tiles,
// k_conv_kw, or the 256-row tiles when it has >= 256 of them.
// Measured at 4 objects per GPU (profiles/r06_tiles_microbench.txt): 3x3x3 launches -5 ... -15 % on 128-row tiles with half the
// slabs of the 256-row split; 1x1 launches with 14-105 K units -20 ... -25 % on k_conv_kw; wide 1x1 launches -15 ... -25 % on
// 64-row producer/consumer tiles (no split).
bool few_eligible(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const RefSize& R) {
    if (!o.conv_few || !L.ws || !R.small) return false;
    // the GEGLU projection of a small problem (never split: its epilogue needs the whole sum): 64-row producer/consumer tiles
    // instead of the non-specialised 64-row kernel (672 -> 5376 at 16x4x4 with 4 objects)
    if (a.epilogue == ES_EPI_GEGLU) return a.mode != ES_CONV_UP_HW && a.mode != ES_CONV_UP_DHW && a.taps == 1 && a.splitk <= 0 && L.wg.t128 < 320;
    return a.splitk < 0 && L.can_split;
}
// a K-short 1x1 launch whose reference problem is one round of 64 x 112 tiles (with 384 of them the 64-row tiles win)
bool few_kstreams_fit(const es_conv_args& a, const LaunchSize& L, const RefSize& R) {
    return a.epilogue != ES_EPI_GEGLU && a.taps == 1 && L.nks < 112 && R.hg.t64h <= 272 && L.nks >= 12;
}
int split_few_plain(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const RefSize& R) {
    if (!few_eligible(a, o, L, R)) return 0;
    if (a.epilogue == ES_EPI_GEGLU || (a.taps == 1 && L.nks < 112)) return few_kstreams_fit(a, L, R) ? 0 : 1;
    const long h128 = R.hg.t128;
    int s2 = (int)((256 + h128 / 2) / h128);
    s2 = s2 < 1 ? 1 : (s2 > 8 ? 8 : s2);
    // (the split that fills the chip best must fit ONE round of workgroups: 96 tiles of 128 rows -- the 16x4x4 level at 16
    //  objects -- want S = 3 = 288 workgroups; with S = 2 the 256-row tiles' S = 5 is the better use of the chip, 91 against 96 us)
    const bool one_round = h128 * s2 <= 272;
    s2 = keep_units(s2, L.nks, 24);
    // (very long K on a handful of tiles -- 1344 -> 672 at 16x4x4 with 4 objects -- stays on the 256-row tiles with S = 16;
    //  an UNSPLIT launch that would leave a quarter of the CUs idle -- 192 tiles of 128 rows: the 16x4x4 level at 32 objects --
    //  stays on the 256-row tiles with S = 2: the same workgroup count on the tile that moves fewer bytes, 169 against 179 us)
    return !(L.nks >= 800 && h128 * 8 < 256) && one_round && (s2 >= 2 || h128 >= 224) ? s2 : 0;
}
int split_few_kstreams(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const RefSize& R) {
    if (!few_eligible(a, o, L, R) || !few_kstreams_fit(a, L, R)) return 0;
    // on k_conv_kw the four K ranges meet in LDS: no slabs, no reduction launch.  A launch with enough 256-row tiles, or more than
    // three rounds of 64 x 112 tiles, cuts the same four ranges over workgroups
    return L.wg.t256 < 256 && L.wg.t64h <= 768 ? 1 : 4;
}

int split_caller(const es_conv_args& a, const RouteOptions&, const LaunchSize& L, const RefSize&) { return a.splitk > 0 ? caller_split(a, L) : 0; }

// Small problems (few objects per GPU: the strong-scaling regime, or the 16x4x4 level): fewer than 256 tiles of 256 rows.  The
// 128- / 64-row kernels stream the weight tile twice / four times per 256 rows and cost 0.9 us per K unit and workgroup
// against 0.64 us for a 256-row producer/consumer tile, so keep the 256-row tiles and split K until about one workgroup per
// CU runs (A/B ES_CONV_WSSPLIT: shape step 21.44 -> 20.76 ms at 32 objects, 13.69 -> 12.61 / 9.22 -> 8.32 / 6.68 -> 6.27 ms at 16 / 8 / 4).
// (the tile count of the WHOLE problem -- a shard with O_hint makes the choice the unsharded run makes, so its partial sums are
//  cut in the same places and the results stay bit-identical; it then simply runs fewer workgroups)
int split_rows256(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const RefSize& R) {
    if (!(L.ws && a.epilogue != ES_EPI_GEGLU && a.splitk < 0 && L.can_split && R.small && o.conv_wssplit != 0)) return 0;
    const long wst = o.conv_wss_target;                            // workgroup target of the split (256 = one round)
    const int s2 = keep_units((int)std::min(wst / R.hg.t256, (long)R.slab_cap), L.nks, 24);
    return s2 >= 2 && R.hg.t256 * s2 >= 160 ? s2 : 0;
}

// Tiny K-short problems (the transformer linears at <= 8 objects per GPU: e.g. 1024 rows x 672 columns, 21 K units): even the
// 64-row tiles give only a few dozen workgroups, each a lone, latency-bound chain of K units (22-30 us for < 1 GFLOP).
// Such launches go to k_linear_deep (7-slot ring issued at entry, no split, no reduction kernel) when they are plain
// linears of at most ONE round of 64-row tiles (140 KB of LDS = one workgroup per CU: with more tiles than CUs the 3-slot kernel's two
// workgroups per CU win; stand-alone at 4 objects: 448 -> 448 19.7 -> 12.5 us, 672 -> 2016 21.4 -> 13.8, but 448 -> 1344 with 384
// tiles 16.7 -> 21.3); split_tiny remains for the shapes it does not take (fused skip phase, 27 taps, more tiles).
// (with at most 28 K units the automatic split it stands in for would be 1 as well: every part of a split keeps 24)
int split_deep(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const RefSize& R) {
    return a.splitk <= 0 && R.small && R.hg.t64 <= 256 && a.taps == 1 && !a.a2 && a.mode == ES_CONV_SAME && L.nks >= 4 && L.nks <= 28 &&
           a.out_ld >= 0 && L.M * (long)a.Cin * 2 < (1L << 31) && o.conv_deep != 0 ? 1 : 0;
}
// ... the others: split K over 64-row tiles until about one workgroup per CU runs (>= 5 units per split)
int split_tiny(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const RefSize& R) {
    if (!(a.splitk < 0 && L.can_split && o.conv_force256 != 1 && R.hg.t256 < 256 && R.hg.t128 < 128 && R.hg.t64 < 256 && L.nks >= 10 &&
          o.conv_tinysplit != 0)) return 0;
    const int s3 = (int)std::min(std::min((256 + R.hg.t64 - 1) / R.hg.t64, (long)R.slab_cap), (long)(L.nks / 5));
    return s3 >= 2 ? s3 : 0;
}

// tile quantisation: e.g. 384 workgroups of 256 rows on 256 CUs = 2 rounds, the second half empty.  Split K by
// the smallest factor that fills the last round (>= 95 %) if the plain launch wastes more than 20 %.
int split_fill256(const es_conv_args& a, const RouteOptions&, const LaunchSize& L, const RefSize& R) {
    const long hg256 = R.hg.t256;
    if (!(a.splitk < 0 && L.can_split && hg256 >= 256)) return 0;
    const long r1 = (hg256 + 255) / 256;
    if ((double)hg256 / (double)(r1 * 256) < 0.8)
        for (int s2 = 2; s2 <= 4; ++s2) {
            const long w = hg256 * s2;
            if ((double)w / (double)(((w + 255) / 256) * 256) >= 0.95 && L.nks / s2 >= 48) return s2;
        }
    return 0;
}

// ~3 workgroups per CU: enough for the dynamic scheduler to balance the tail, few enough that the epilogue
// and the reduction (S slabs of M x N floats) stay small (measured, tools/microbench_small.py: M = 8192
// rows best at S = 4, 16384 rows at S = 2-3, 1024-4096 rows at S = 8)
int split_auto128(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const RefSize& R) {
    if (!(a.splitk < 0 && L.can_split && o.conv_force256 != 1 && R.hg.t256 < 256 && R.hg.t128 < 512)) return 0;
    const long want = (768 + R.hg.t128 / 2) / R.hg.t128;
    const int S = keep_units((int)std::min(std::max(want, 1L), 8L), L.nks, 24);
    return S > 1 ? S : 0;
}
int split_none(const es_conv_args&, const RouteOptions&, const LaunchSize&, const RefSize&) { return 1; }

// The rules in the order they are tried: the first whose function answers an S takes the launch.  (forced_tile first: the tools'
// options pre-empt everything; few_* before rows256 / deep / tiny / auto128, which all want the same small problems; fill256 is
// for problems none of those take -- 256 tiles of 256 rows or more.)
const struct { SplitRule rule; int (*split)(const es_conv_args&, const RouteOptions&, const LaunchSize&, const RefSize&); } kSplitRules[] = {
    {SplitRule::forced_tile, split_forced_tile}, {SplitRule::few_plain, split_few_plain}, {SplitRule::few_kstreams, split_few_kstreams},
    {SplitRule::caller, split_caller},           {SplitRule::rows256, split_rows256},     {SplitRule::deep, split_deep},
    {SplitRule::tiny, split_tiny},               {SplitRule::fill256, split_fill256},     {SplitRule::auto128, split_auto128},
    {SplitRule::none, split_none},
};
void choose_split(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const RefSize& R, ConvRoute* r) {
    for (const auto& k : kSplitRules)
        if (const int S = k.split(a, o, L, R)) {
            r->rule = k.rule;
            r->S = r->slabs = S;
            return;
        }
}

// ---- step 6: the tile that realises the split, and its grid.  From (rule, launch size, options): nothing of the reference problem ----
// rows of the tile: 256 / 128 / 64; 0: k_conv_kw (few_kstreams with the K streams inside the workgroup)
int few_tile_rows(const es_conv_args& a, const LaunchSize& L, const ConvRoute& r) {
    if (L.wg.t256 >= 256) return 256;                              // enough 256-row tiles: they take the split as it is
    if (r.rule == SplitRule::few_kstreams) return r.S == 1 ? 0 : 128;
    return a.taps == 1 && r.S == 1 ? (L.wg.t128 >= 320 ? 128 : 64) : 128;
}
int tile_rows(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, const ConvRoute& r) {
    const bool no256 = o.conv_tile == 128, force256 = o.conv_force256 == 1;
    switch (r.rule) {
    case SplitRule::few_plain:
    case SplitRule::few_kstreams: return few_tile_rows(a, L, r);
    case SplitRule::rows256: return 256;
    case SplitRule::tiny: return 64;
    default: break;
    }
    // (conv_force256 puts an unsplit launch, or one split to fill its last round, on 256-row tiles whatever its size)
    if (!no256 && (L.wg.t256 >= 256 || (force256 && (r.S == 1 || r.rule == SplitRule::fill256)))) return 256;
    return L.wg.t128 >= 512 || r.S > 1 ? 128 : 64;
}

// tools: the tile the options name, built or not
void forced_tile(const RouteOptions& o, const LaunchSize& L, ConvRoute* r) {
    const unsigned uy = (unsigned)L.ntn;
    if (const int ks = L.forced_ks) {
        r->kernel = ks == 4 ? ConvKernel::kw_4_1 : ks == 2 ? ConvKernel::kw_2_2 : ConvKernel::none;
        snprintf(r->unbuilt, sizeof(r->unbuilt), "conv_kw_ks=%d (2 or 4)", ks);
        r->gx = (unsigned)((L.M + 63) / 64); r->gy = ks == 4 ? 2 * uy : uy;
        return;
    }
    const int bm = L.forced_bm, np = o.conv_st_np, ns = o.conv_st_ns;
    if (bm == 64 && np == 4 && ns == 3) r->kernel = ConvKernel::ws_64_4_4_3;
    else if (bm == 64 && np == 4 && ns == 6) r->kernel = ConvKernel::ws_64_4_4_6;
    else if (bm == 128 && np == 4 && ns == 3) r->kernel = ConvKernel::ws_128_4_4_3;
    else if (bm == 128 && np == 8 && ns == 3) r->kernel = ConvKernel::ws_128_4_8_3;
    else if (bm == 128 && np == 8 && ns == 5) r->kernel = ConvKernel::ws_128_4_8_5;
    else snprintf(r->unbuilt, sizeof(r->unbuilt), "conv_st_bm=%d conv_st_np=%d conv_st_ns=%d is not a built tile", bm, np, ns);
    r->gx = (unsigned)((L.M + bm - 1) / bm); r->gy = uy;
}

// the 256-row tiles: k_linear_ws, the producer/consumer kernel in one of its three forms, or the non-specialised kernel
void tile_256(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, ConvRoute* r) {
    r->gx = (unsigned)((L.M + 255) / 256);
    // 1x1 / linear launches with several column tiles: one workgroup walks NCB column tiles of its row tile (k_linear_ws)
    // (ES_CONV_LINWS: A/B switch, 0 = off)
    if (L.ws && a.taps == 1 && !a.a2 && a.mode == ES_CONV_SAME && r->S == 1 && L.ntn >= 2 && o.env_linws)
        for (const int ncb : {8, 6, 4, 3, 2})
            if (L.ntn % ncb == 0 && (long)r->gx * (L.ntn / ncb) >= 256) {
                r->kernel = ConvKernel::linear_ws;
                r->ncb = ncb; r->gy = (unsigned)(L.ntn / ncb);
                return;
            }
    if (!(L.ws && (!r->geglu || !r->upm))) { r->kernel = ConvKernel::lean_256; return; }
    // 3x3x3 SAME convs on volumes with W <= 16: the A tile of a (chunk, kd, kh) group staged once, the kw = -1 / +1 operands
    // shifted in registers (k_conv_ws3; bit-identical to k_conv_ws).  ES_CONV_A3 = 0 / 1: timing-only A/B switch
    const bool a3 = o.env_a3 && a.taps == 27 && a.mode == ES_CONV_SAME && !a.a2 && a.W <= 16 && a.W >= 4;
    r->kernel = a3 ? ConvKernel::ws3 : ConvKernel::ws_256_8_4_3;
    // An UP_HW launch that carries its folded image (w2, read by no other UP launch: they have no skip phase) multiplies 12 folded
    // taps per chunk instead of 27 (k_conv_ws_fold) -- only here: an unsplit launch of a non-sharded plan (O_hint == 0: the
    // canonical and the sharded arithmetic stay the 27-tap one) whose 256-row tiles are each one parity class of one object.
    // Other products than the 27-tap route's (the folded weights are rounded after the sum): not bit-equal to it.
    if (a3 || !(a.mode == ES_CONV_UP_HW && a.w2 && !a.a2 && r->S == 1 && a.O_hint == 0 && a.H >= 2 && a.W >= 2 &&
                ((long)a.D * r->g.Hi * r->g.Wi) % 256 == 0)) return;
    r->kernel = ConvKernel::ws_256_up_fold;
    // three column tiles, no workspace, on a grid whose last round of 256 workgroups is mostly empty (384 tiles: 75 % of two rounds):
    // 2 workgroups per row tile, each one whole tile and half of the third column tile (k_conv_ws_fold_bal) -- the same
    // sums in the same order, S stays 1
    const long rounds = (L.wg.t256 + 255) / 256;
    if (L.ntn == 3 && !a.workspace && L.M % 256 == 0 && (double)L.wg.t256 / (double)(rounds * 256) < 0.8) {
        r->fold_bal = true;
        r->gy = 2;
    }
}

// Sets kernel, grid and ncb.  Returns whether the tile is one whose epilogue can form gn_stats_out's row-group sums: a
// producer/consumer tile of 256 or 128 rows (64-row waves), one column tile per workgroup
bool choose_tile(const es_conv_args& a, const RouteOptions& o, const LaunchSize& L, ConvRoute* r) {
    r->ncb = 1;
    r->gy = (unsigned)L.ntn; r->gz = (unsigned)r->S;
    if (r->rule == SplitRule::forced_tile) { forced_tile(o, L, r); return L.forced_bm == 128; }
    if (r->rule == SplitRule::deep) {
        r->kernel = ConvKernel::linear_deep;
        r->gx = (unsigned)((L.M + 63) / 64);
        return false;
    }
    const bool few = r->rule == SplitRule::few_plain || r->rule == SplitRule::few_kstreams;
    const int rows = tile_rows(a, o, L, *r);
    switch (rows) {
    case 256: tile_256(a, o, L, r); return L.ws && r->ncb == 1;
    case 128: r->kernel = few ? ConvKernel::ws_128_4_8_5 : ConvKernel::lean_128; break;
    case 64: r->kernel = few ? ConvKernel::ws_64_4_4_3 : ConvKernel::lean_64; break;
    default: r->kernel = ConvKernel::kw_4_1; r->gy = 2 * (unsigned)L.ntn; break;       // (64 rows x 112 columns per workgroup)
    }
    r->gx = (unsigned)((L.M + (rows ? rows : 64) - 1) / (rows ? rows : 64));
    return few && rows == 128;
}

// ---- step 7: who forms the GroupNorm sums, and the reduction behind a split ------------------------------------------------------
void route_flags(const es_conv_args& a, bool stats_tile, ConvRoute* r) {
    const int V = a.D * a.H * a.W;
    // the producer/consumer 256-row kernel forms the row-group sums of gn_stats_out in its epilogue; every other route runs
    // k_rowgroup_stats over the finished output
    r->epi_stats = stats_tile && !r->geglu && r->S == 1 && (a.out_f32 || a.out_f16) && a.N % 4 == 0 && a.out_ld % 4 == 0 && V % 64 == 0;
    // a split launch can form the next GroupNorm's per-tile partial sums in its reduction kernel (gn_part_out)
    // (the few-objects routes: from the REFERENCE problem's decision -- K streams inside the workgroup have no reduction launch,
    //  whatever kernel realises the split in this launch)
    r->part_ok = r->S > 1 && r->rule != SplitRule::few_kstreams && a.out_f32 && !r->ncdhw && a.N % 4 == 0 && a.N <= 2048 && a.out_ld == a.N &&
                 a.gn_part_groups > 0 && a.gn_part_groups <= 64 && a.N % a.gn_part_groups == 0;
    const bool want_stats = a.gn_stats_out != nullptr;
    r->stats = want_stats && r->epi_stats;
    r->stats_pass = want_stats && !r->epi_stats;   // (every kernel chosen under epi_stats has the epilogue that forms the sums)
    if (r->S > 1) {
        r->reduce = a.gn_part_out && r->part_ok ? ConvReduce::gn_part : ConvReduce::plain;
        if (r->reduce == ConvReduce::gn_part) r->vt = gn_voxel_tile(ref_objects(a), V);
    }
}

}  // namespace

es_conv_args conv_chunk_args(const es_conv_args& a, const ConvGeom& g, long o0, long n) {
    const long V = (long)a.D * a.H * a.W;
    es_conv_args c = a;
    c.O = (int32_t)n;
    c.O_hint = a.O_hint < 0 ? a.O_hint : (a.O_hint > a.O ? a.O_hint : a.O);
    c.a = (const char*)a.a + o0 * obj_bytes_in(a, g);
    if (a.a2) c.a2 = (const char*)a.a2 + o0 * obj_bytes_in2(a);
    if (a.rowvec) c.rowvec = a.rowvec + o0 * a.rowvec_ld;
    if (a.out_ld < 0) {                                            // NCDHW
        c.out_f32 = a.out_f32 + o0 * a.N * V;
    } else {
        if (a.res) c.res = a.res + o0 * V * a.out_ld;
        if (a.out_f32) c.out_f32 = a.out_f32 + o0 * V * a.out_ld;
        if (a.out_f16) c.out_f16 = (char*)a.out_f16 + o0 * V * a.out_ld * 2;
    }
    c.gn_stats_out = c.gn_part_out = nullptr;
    return c;
}

int conv_route(const es_conv_args& a, const RouteOptions& o, ConvRoute* r) {
    *r = ConvRoute{};
    if (int err = route_geometry(a, r)) return err;
    if (int err = route_chunks(a, o, r)) return err;
    if (r->omax || route_direct(a, o, r)) return 0;
    ES_REQUIRE(!a.gn_stats_out || ((a.out_f32 || a.out_f16) && !r->ncdhw && a.N % 4 == 0 && a.out_ld % 4 == 0 && (a.D * a.H * a.W) % 64 == 0 &&
                                   a.epilogue == ES_EPI_NONE),
               "es_conv_mfma_f16: gn_stats_out needs a channels-last output, N %% 4 == 0 and voxels per object %% 64 == 0");
    r->upm = a.mode == ES_CONV_UP_HW || a.mode == ES_CONV_UP_DHW;
    r->geglu = a.epilogue == ES_EPI_GEGLU;
    ES_REQUIRE(!r->upm || (!a.a2 && a.taps == 27), "es_conv_mfma_f16: nearest-up modes take 3x3x3 convs without a fused skip");
    const LaunchSize L = launch_size(a, o, *r);
    choose_split(a, o, L, ref_size(a, o), r);
    route_flags(a, choose_tile(a, o, L, r), r);
    return 0;
}

// ---- the host-only queries: readers of one route under the process's options.  They launch nothing. ------------------------------
extern "C" int es_conv_route_of(const es_conv_args* a, es_conv_route_info* out) {
    ConvRoute r;
    if (conv_route(*a, es_route_options(), &r) != 0) return -1;
    *out = es_conv_route_info{(int32_t)r.kernel, r.gx, r.gy, r.gz, (int32_t)r.lds, r.S, r.slabs, r.ncb, (int32_t)r.omax,
                              (int32_t)r.epi_stats, (int32_t)r.stats, (int32_t)r.stats_pass, (int32_t)r.part_ok, (int32_t)r.reduce, r.vt,
                              (int32_t)r.fold_bal};
    return 0;
}
// 1 when es_conv_mfma_f16(args) would form gn_stats_out inside its own epilogue (the planner only asks a conv for the sums then:
// behind any other route they would cost a pass over the output, i.e. what the GroupNorm's own statistics pass costs), 0 when
// not, -1 on invalid arguments
extern "C" int es_conv_emits_gn_stats(const es_conv_args* a) {
    es_conv_route_info i;
    return es_conv_route_of(a, &i) == 0 ? i.epi_stats : -1;
}
// 1 when a split launch's reduction kernel can form the next GroupNorm's per-tile partial sums (gn_part_out), 0 when not, -1 on
// invalid arguments
extern "C" int es_conv_emits_gn_part(const es_conv_args* a) {
    es_conv_route_info i;
    return es_conv_route_of(a, &i) == 0 ? i.part_ok : -1;
}
// The number of fp32 slabs [S][M][N] es_conv_mfma_f16(args) writes into args->workspace (1: none -- no split, or K split inside the
// workgroup), -1 on invalid arguments: the planner sizes the workspace with it
extern "C" int es_conv_split_of(const es_conv_args* a) {
    es_conv_route_info i;
    return es_conv_route_of(a, &i) == 0 ? i.slabs : -1;
}
// The name of the kernel es_conv_mfma_f16(args) would launch (the ConvKernel enumerator's spelling; "chunked" for a launch over the
// 2 GiB descriptor limit, whose chunks are routed one by one; "none" for forcing options that name a tile that is not built),
// written into name_out (cap bytes, always terminated); returns the split of K over workgroups (ConvRoute::S, >= 1; a chunked
// launch: of a full chunk), -1 on invalid arguments: tests assert with it that the kernel they mean is the one that ran
extern "C" int es_conv_kernel_of(const es_conv_args* a, char* name_out, int cap) {
    es_conv_route_info i;
    if (es_conv_route_of(a, &i) != 0) return -1;
    if (name_out && cap > 0) snprintf(name_out, (size_t)cap, "%s", i.omax ? "chunked" : kConvKernelName[i.kernel]);
    return i.S > 1 ? i.S : 1;
}
// 1 when es_conv_mfma_f16(args) takes the folded route on its balanced schedule (ConvRoute::fold_bal: three column tiles on a grid
// whose last round is mostly empty -- two workgroups per row tile, each one tile and a half), 0 when not, -1 on invalid arguments;
// the kernel name and the split that es_conv_kernel_of reports do not depend on it
extern "C" int es_conv_fold_balanced(const es_conv_args* a) {
    es_conv_route_info i;
    return es_conv_route_of(a, &i) == 0 ? i.fold_bal : -1;
}

// ---- es_groupnorm_vol: the launch decisions.  Voxel-tile sizes by workgroup count: small problems (few objects per GPU when sharded)
// get smaller tiles; tile sizes from the whole problem when this launch is a shard (O_hint > O), from the reference shard when
// O_hint < 0. ---------------------------------------------------------------------------------------------------------------------
int gn_route(const es_gn_args& a, const RouteOptions& o, GnRoute* r) {
    const int C = a.C1 + a.C2;
    ES_REQUIRE(a.groups > 0 && C > 0 && C % a.groups == 0 && C <= 2048 && a.groups <= 64, "es_groupnorm_vol: C=%d groups=%d", C, a.groups);
    ES_REQUIRE(a.C1 % 8 == 0 && a.C2 % 8 == 0, "es_groupnorm_vol: channel counts must be multiples of 8 (%d,%d)", a.C1, a.C2);
    ES_REQUIRE(a.O > 0 && a.V > 0, "es_groupnorm_vol: O=%d V=%d", a.O, a.V);
    ES_REQUIRE(a.stats != nullptr, "es_groupnorm_vol: stats scratch missing");
    const long Oh = a.O_hint < 0 ? -(long)a.O_hint : (long)(a.O_hint > a.O ? a.O_hint : a.O);
    r->vt = gn_voxel_tile(Oh, a.V);
    r->ntiles = (a.V + r->vt - 1) / r->vt;
    const bool from_rg = a.stats1 && (!a.x2 || a.stats2) && a.V % 64 == 0 && (a.x1_is_f16 || o.gn_rg != 0);
    ES_REQUIRE(!a.x1_is_f16 || (from_rg && !a.x2 && !a.raw_f16),
               "es_groupnorm_vol: an f16 source needs the producer's row-group sums (stats1), one source, no raw copy");
    ES_REQUIRE(!a.part_in || (!from_rg && !a.x2), "es_groupnorm_vol: part_in needs one source and no row-group sums");
    r->src = from_rg ? GnStats::rowgroup : a.part_in ? GnStats::part_in : GnStats::pass;
    r->partial_gx = r->partial_gy = r->fin_gx = r->fin_gy = 0;
    if (r->src == GnStats::pass) { r->partial_gx = (unsigned)r->ntiles; r->partial_gy = (unsigned)a.O; }
    int vpb = 32;
    while (vpb > 8 && (long)a.O * ((a.V + vpb - 1) / vpb) < 512) vpb >>= 1;
    while (vpb < 1024 && (long)a.O * ((a.V + vpb - 1) / vpb) > 16384) vpb <<= 1;     // (64^3 volumes: fewer, larger blocks)
    r->vpb = vpb;
    // long tile lists (VQ-VAE decoder at 32^3 / 64^3): the statistics are reduced ONCE per object; the final [O][groups][2] floats
    // sit behind the partials in the caller's scratch (es_gn_args.stats)
    r->finalize = !from_rg && r->ntiles > 128;
    r->fin_off = -1;
    if (from_rg) {                 // statistics from the producers' row-group sums: no pass over x1 / x2
        r->fin_off = 0;
    } else if (r->finalize) {
        // (with part_in the partials live in the PRODUCER's buffer, which has no room behind them: the final statistics go to the
        //  front of the caller's own scratch then.  Until round 6 they were written behind part_in -- 256 bytes past the end of a
        //  buffer that ends on a page boundary was a GPU memory fault at one object per GPU, 16^3 level)
        r->fin_off = a.part_in ? 0 : (long)a.O * r->ntiles * a.groups * 2;
    }
    if (r->fin_off >= 0) { r->fin_gx = (unsigned)a.groups; r->fin_gy = (unsigned)a.O; }
    r->TX = 1 << gn_apply_log2_tx(C >> 3);
    r->apply_gx = (unsigned)((a.V + vpb - 1) / vpb);
    r->apply_gy = (unsigned)a.O;
    return 0;
}

extern "C" int es_groupnorm_route_of(const es_gn_args* a, es_gn_route_info* out) {
    GnRoute r;
    if (gn_route(*a, es_route_options(), &r) != 0) return -1;
    *out = es_gn_route_info{r.vt, r.ntiles, (int32_t)r.src, (int32_t)r.finalize, (int32_t)r.fin_off, r.vpb, r.TX,
                            r.partial_gx, r.partial_gy, r.fin_gx, r.fin_gy, r.apply_gx, r.apply_gy};
    return 0;
}

// ---- es_attention_f16 / es_attention_f32: the instantiation by head dimension and sequence length ----------------------------------
const char* const kAttnKernelName[] = {
    "attention_32_4_1", "attention_32_4_2", "attention_64_4_1", "attention_64_4_2", "attention_96_4_1", "attention_96_4_2", "attention_256_4_1",
    "attention_f32m_64", "attention_f32m_96", "attention_f32_64", "attention_f32_96"
};

int attn_route(const es_attn_args& a, bool fp32, AttnRoute* r) {
    ES_REQUIRE(a.B > 0 && a.Ntok > 0 && a.heads > 0, "es_attention: B=%d Ntok=%d heads=%d", a.B, a.Ntok, a.heads);
    r->lds = 0;
    if (fp32) {
        ES_REQUIRE(a.dhead > 0 && a.dhead <= 96, "es_attention_f32: dhead=%d (<= 96)", a.dhead);
        r->rows = 64;
        r->DP = a.dhead <= 64 ? 64 : 96;
        if (a.dhead % 4 == 0) {
            // round 6: the matrix-instruction kernel (dhead a multiple of 4: the K / V tiles are staged in 16-byte quads): K and V tiles
            // of 64 keys x (DP + 4) floats, and 4 waves x 16 rows x 68 floats of probabilities
            r->kernel = a.dhead <= 64 ? AttnKernel::f32m_64 : AttnKernel::f32m_96;
            r->block = 256;
            r->lds = (size_t)(2 * 64 * (r->DP + 4) + 4 * 16 * 68) * 4;
        } else {
            r->kernel = a.dhead <= 64 ? AttnKernel::f32_64 : AttnKernel::f32_96;
            r->block = 64;
        }
    } else {
        ES_REQUIRE(a.dhead % 4 == 0 && a.dhead <= 256 && a.dhead > 0, "es_attention_f16: dhead=%d (multiple of 4, <= 256)", a.dhead);
        ES_REQUIRE(a.scale > 0.f, "es_attention_f16: scale=%g must be positive (the row maximum is taken over the raw scores)", (double)a.scale);
        const bool big = a.Ntok >= 512 && a.dhead <= 96;       // 128 query rows per workgroup (4 waves x 2 row tiles), else 64 (4 x 1)
        r->rows = big ? 128 : 64;
        r->block = 256;
        if (a.dhead <= 32) { r->DP = 32; r->kernel = big ? AttnKernel::h32_2 : AttnKernel::h32_1; }
        else if (a.dhead <= 64) { r->DP = 64; r->kernel = big ? AttnKernel::h64_2 : AttnKernel::h64_1; }
        else if (a.dhead <= 96) { r->DP = 96; r->kernel = big ? AttnKernel::h96_2 : AttnKernel::h96_1; }
        else { r->DP = 256; r->kernel = AttnKernel::h256_1; }
    }
    r->gx = (unsigned)((a.Ntok + r->rows - 1) / r->rows);
    r->gy = (unsigned)(a.B * a.heads);
    return 0;
}

extern "C" int es_attention_route_of(const es_attn_args* a, int fp32, es_attn_route_info* out) {
    AttnRoute r;
    if (attn_route(*a, fp32 != 0, &r) != 0) return -1;
    es_attn_route_info i{};
    snprintf(i.kernel, sizeof(i.kernel), "%s", kAttnKernelName[(int)r.kernel]);
    i.DP = r.DP; i.rows = r.rows; i.grid_x = r.gx; i.grid_y = r.gy; i.block = r.block; i.lds = (int32_t)r.lds;
    *out = i;
    return 0;
}
