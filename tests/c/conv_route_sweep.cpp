// Stand-alone sweep of the contract of the conv routing unit (echoscene_amd/csrc/es_conv_route.hip, compiled with it as plain C++
// under the host sanitizers by tests/test_conv_route_sweep_cpu.py): what the planner and the workspace contract of echoscene_hip.h
// rely on, for every accepted route of a grid of about 19 M argument sets x option settings.  No GPU, no HIP, no library: only the
// public header.  Exit status 0 and one summary line, or 1 and the first violations.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "echoscene_hip.h"

void es_set_error(const char*, ...) {}          // (the unit reports refused arguments through it; the sweep only counts them)

struct Layer { int cin, n, taps, cin2, epi; };
// the shape UNet's and the VQ-VAE's layers (tests/golden/make_conv_routes.py) and two with ragged column counts
static const Layer LAYERS[] = {
    {224, 224, 27, 0, 0}, {224, 448, 27, 0, 0}, {448, 448, 27, 0, 0}, {448, 672, 27, 0, 0}, {672, 672, 27, 0, 0},
    {672, 672, 27, 672, 0}, {672, 448, 27, 448, 0}, {448, 448, 27, 448, 0}, {448, 224, 27, 224, 0}, {224, 224, 27, 224, 0},
    {224, 16, 27, 0, 0}, {224, 3, 27, 0, 0},
    {224, 448, 1, 0, 0}, {448, 672, 1, 0, 0}, {672, 672, 1, 672, 0}, {448, 448, 1, 224, 0},
    {448, 448, 1, 0, 0}, {672, 672, 1, 0, 0}, {448, 1344, 1, 0, 0}, {672, 2016, 1, 0, 0},
    {448, 3584, 1, 0, 1}, {672, 5376, 1, 0, 1}, {1792, 448, 1, 0, 0}, {2688, 672, 1, 0, 0}, {1344, 672, 1, 0, 0},
    {64, 64, 27, 0, 0}, {64, 128, 27, 0, 0}, {128, 128, 27, 0, 0}, {128, 256, 27, 0, 0}, {256, 256, 27, 0, 0},
    {64, 4, 27, 0, 0}, {64, 1, 27, 0, 0}, {256, 4, 27, 0, 0}, {64, 128, 1, 0, 0}, {128, 256, 1, 0, 0}, {256, 4, 1, 0, 0},
    {32, 232, 27, 0, 0}, {160, 232, 1, 0, 0}};
static const int VOLS[][3] = {{1, 1, 1}, {16, 4, 4}, {16, 8, 8}, {16, 16, 16}, {64, 64, 64}, {128, 128, 128}};
static const int OBJ[] = {1, 4, 16, 32, 513, 65535};
static const int HINT[] = {0, -4, 32};
static const int SPLITK[] = {-1, 0, 2, 16, 1000};
static const char* SETTINGS[] = {"", "conv_few=0", "conv_wssplit=0", "conv_wss_target=512", "conv_tile=128", "conv_force256=1", "conv_ws=0", "conv_deep=0",
                                 "conv_tinysplit=0", "conv_st_bm=64", "conv_st_bm=128,conv_st_np=8", "conv_kw_ks=4", "conv_kw_ks=2"};

static long g_bad = 0;
static void violated(const char* what, const char* setting, const es_conv_args& a, const es_conv_route_info& r) {
    if (g_bad++ >= 10) return;
    fprintf(stderr, "VIOLATED: %s\n  options \"%s\" O=%d %dx%dx%d Cin=%d N=%d taps=%d mode=%d Cin2=%d epilogue=%d splitk=%d O_hint=%d workspace=%d out_ld=%d w2=%d\n"
            "  route: kernel=%d grid=(%u,%u,%u) S=%d slabs=%d omax=%d reduce=%d\n", what, setting, a.O, a.D, a.H, a.W, a.Cin, a.N, a.taps, a.mode, a.Cin2,
            a.epilogue, a.splitk, a.O_hint, a.workspace != nullptr, a.out_ld, a.w2 != nullptr, r.kernel, r.grid_x, r.grid_y, r.grid_z, r.S, r.slabs, r.omax, r.reduce);
}
#define CHECK(cond) do { if (!(cond)) violated(#cond, setting, a, r); } while (0)

static void check(const char* setting, bool tools, const es_conv_args& a, const es_conv_route_info& r) {
    if (r.omax > 0) {                                           // launched chunk by chunk: each chunk has a route of its own
        CHECK(r.kernel == 0 && r.omax < a.O);
        return;
    }
    // the reference problem's rows x columns: 16 slabs for small outputs, else 8 (es_conv_args.splitk)
    const long Oh = a.O_hint < 0 ? -(long)a.O_hint : (a.O_hint > a.O ? a.O_hint : a.O);
    const long MhN = Oh * a.D * a.H * a.W * a.N;
    if (a.splitk < 0) CHECK(r.slabs <= (MhN <= (1L << 22) ? 16 : 8));
    if (a.splitk > 1) CHECK(r.slabs <= a.splitk);
    if (!a.workspace) CHECK(r.S == 1 && r.slabs <= 1);
    if (r.S > 1) CHECK(r.slabs == r.S && r.reduce != 0);
    if (r.S == 1) CHECK(r.reduce == 0);
    CHECK(r.grid_x >= 1 && r.grid_y >= 1 && r.grid_z >= 1 && r.grid_y <= 65535 && r.grid_z <= 65535);
    if (!tools) CHECK(r.kernel != 0);
}

static void set_options(const char* list, const char* sep) {      // "name=value<sep>name=value..."
    char buf[1024];
    snprintf(buf, sizeof(buf), "%s", list);
    for (char* kv = strtok(buf, sep); kv; kv = strtok(nullptr, sep)) {
        char* eq = strchr(kv, '=');
        *eq = 0;
        if (es_vol_set_option(kv, atoi(eq + 1)) != 0) { fprintf(stderr, "unknown option %s\n", kv); exit(2); }
    }
}

int main() {
    long n = 0, refused = 0, chunked = 0;
    char defaults[1024];
    es_vol_options(defaults, sizeof(defaults));
    for (const char* setting : SETTINGS) {
        set_options(defaults, ";");
        set_options(setting, ",");
        const bool tools = strstr(setting, "conv_st_bm") || strstr(setting, "conv_kw_ks");
        for (const Layer& l : LAYERS) for (const auto& vol : VOLS) for (int O : OBJ) for (int hint : HINT) for (int sk : SPLITK)
        for (int mode = 0; mode < 6; ++mode) for (int wsp = 0; wsp < 2; ++wsp) for (int out = 0; out < 3; ++out) for (int extra = 0; extra < 2; ++extra) {
            es_conv_args a;
            memset(&a, 0, sizeof(a));
            a.a = (const void*)0x1000; a.w = (const void*)0x2000; a.bias = (const float*)0x5000;      // (never dereferenced)
            a.O = O; a.D = vol[0]; a.H = vol[1]; a.W = vol[2]; a.Cin = l.cin; a.N = l.n; a.taps = l.taps; a.mode = mode; a.epilogue = l.epi;
            a.splitk = sk; a.O_hint = hint;
            if (l.cin2) { a.a2 = (const void*)0x1100; a.w2 = (const void*)0x2100; a.Cin2 = l.cin2; }
            const int o = l.epi && out == 0 ? 1 : out;          // (the GEGLU epilogue writes fp16 only)
            a.out_ld = o == 2 ? -1 : (l.epi ? l.n / 2 : l.n);
            if (o == 0 || o == 2) a.out_f32 = (float*)0x3000;
            if (o == 1) a.out_f16 = (void*)0x4000;
            if (wsp) a.workspace = (void*)0x6000;
            if (extra) {                                        // the folded weight image and the planner's GroupNorm requests
                a.w2 = (const void*)0x2100;
                a.gn_stats_out = (float*)0x7000; a.gn_part_out = (float*)0x8000; a.gn_part_groups = 32;
            }
            es_conv_route_info r;
            ++n;
            if (es_conv_route_of(&a, &r) != 0) { ++refused; continue; }
            chunked += r.omax > 0;
            check(setting, tools, a, r);
        }
    }
    printf("%ld routes: %ld refused, %ld chunked, %ld violations\n", n, refused, chunked, g_bad);
    return g_bad != 0 || n - refused < n / 4;                  // (a sweep that is refused nearly everywhere checks nothing)
}
