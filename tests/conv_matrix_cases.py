"""The conv kernel x mode matrix: the cases, and for each launch of a case the kernel and the split of K that the routing rule gives it
(es_conv_kernel_of).  Shared by tests/test_conv_matrix_cpu.py (the routes, no GPU) and tests/test_hip_conv_matrix.py (the same launches
run, against fp64).  A plain module: no fixtures, no test.

A case is a dict: name, O, dims (the OUTPUT grid), taps, Cin, N, mode, Cin2 (fused 1x1 skip phase, 0: none), rowvec, res, out
('both': fp32 + f16 channels-last, 'f32', 'f16', 'ncdhw'), geglu, stats (the row-group sums are asked for as well), and `routes`: a list
of Route(options, splitk, kernel, S) -- the route options set through es_vol_set_option (everything else at its default), the
es_conv_args.splitk of the launch (None: what the planner passes when the caller says nothing) and the expected answer.

The families (3x3x3, 64 -> 232 columns: two 224-column tiles with a ragged second, 112 + 112 + 8 for k_conv_kw):
  A  5 objects of 4x4x8: 128 voxels per object, 640 rows -- 256-row tiles straddle objects, the last one is ragged; per-object vector
  B  5 objects of 2x4x4:  32 voxels per object, 160 rows -- the last 64- and 128-row tiles are ragged; no per-object vector (the
     producer/consumer kernels take one only when a wave's 64 rows lie in one object)
each in all six conv modes, and with the fused skip phase in the four modes that take one."""
import collections
import os

SAME, DOWN_HW, UP_HW, UP_DHW, DOWN_DHW, DOWN_DHW_P01 = range(6)
MODE_NAMES = {SAME: 'same', DOWN_HW: 'down_hw', UP_HW: 'up_hw', UP_DHW: 'up_dhw', DOWN_DHW: 'down_dhw', DOWN_DHW_P01: 'down_dhw_p01'}
UP_MODES = (UP_HW, UP_DHW)

# every value of the library's ConvKernel enum (csrc/es_conv_route.h), 'none' excluded
KERNELS = ('small_n', 'small_n_tiled', 'n16', 'kw_4_1', 'kw_2_2', 'ws_256_8_4_3', 'ws_64_4_4_3', 'ws_64_4_4_6', 'ws_128_4_4_3',
           'ws_128_4_8_3', 'ws_128_4_8_5', 'ws3', 'linear_ws', 'linear_deep', 'lean_256', 'lean_128', 'lean_64')
# the kernels whose operand addressing handles the conv modes (k_conv_lean, k_conv_ws, k_conv_kw): each must be reached in all six
MODE_KERNELS = ('lean_64', 'lean_128', 'lean_256', 'ws_256_8_4_3', 'ws_64_4_4_3', 'ws_64_4_4_6', 'ws_128_4_4_3', 'ws_128_4_8_3',
                'ws_128_4_8_5', 'kw_4_1', 'kw_2_2')
# the kernels that form the row-group sums of gn_stats_out in their own epilogue (es_conv_emits_gn_stats == 1), unsplit
STATS_KERNELS = ('ws_256_8_4_3', 'ws3', 'ws_128_4_4_3', 'ws_128_4_8_3', 'ws_128_4_8_5')

Route = collections.namedtuple('Route', 'options splitk kernel S')

NO_FEW = {'conv_few': 0, 'conv_wssplit': 0, 'conv_tinysplit': 0, 'conv_deep': 0}


def expected_kernel(name):
    """ES_CONV_A3=0 (read once per process; test_conv_alternate_kernels sets it for its subprocess) sends k_conv_ws3's launches to the
    256-row k_conv_ws tile: the same K order, the same bits."""
    return 'ws_256_8_4_3' if name == 'ws3' and os.environ.get('ES_CONV_A3') == '0' else name


def input_dims(mode, dims):
    D, H, W = dims
    return {SAME: (D, H, W), DOWN_HW: (D, 2 * H, 2 * W), UP_HW: (D, H // 2, W // 2), UP_DHW: (D // 2, H // 2, W // 2),
            DOWN_DHW: (2 * D, 2 * H, 2 * W), DOWN_DHW_P01: (2 * D, 2 * H, 2 * W)}[mode]


def family_routes(mode, skip):
    """the route table of both families (the same for every mode but for k_conv_ws3, which takes SAME launches without a skip)"""
    a3 = mode == SAME and not skip
    auto64 = 11 if skip else 10                                  # 54 (+ 3) K units, >= 5 per split
    r = [Route({}, None, 'ws_128_4_8_5', 2),
         Route({'conv_ws': 0}, None, 'lean_64', auto64),
         Route({'conv_force256': 1}, None, 'ws3' if a3 else 'ws_256_8_4_3', 1),
         Route({'conv_ws': 0, 'conv_force256': 1}, None, 'lean_256', 1),
         Route({'conv_st_bm': 64}, None, 'ws_64_4_4_3', 1),
         Route({'conv_st_bm': 64, 'conv_st_ns': 6}, None, 'ws_64_4_4_6', 1),
         Route({'conv_st_bm': 128}, None, 'ws_128_4_4_3', 1),
         Route({'conv_st_bm': 128, 'conv_st_np': 8}, None, 'ws_128_4_8_3', 1),
         Route({'conv_st_bm': 128, 'conv_st_np': 8, 'conv_st_ns': 5}, None, 'ws_128_4_8_5', 1),
         Route({'conv_kw_ks': 4}, None, 'kw_4_1', 1),
         Route({'conv_kw_ks': 2}, None, 'kw_2_2', 1),
         Route(NO_FEW, None, 'lean_128', 2)]
    r += [Route({}, S, 'lean_128', S) for S in (2, 3, 4, auto64)]             # the plain splits the classes below are compared with
    r += [Route({'conv_st_bm': 64}, S, 'ws_64_4_4_3', S) for S in (2, 3, 4)]
    return r


def _family(fam, mode, skip):
    O, dims, rowvec = {'A': (5, (4, 4, 8), True), 'B': (5, (2, 4, 4), False)}[fam]
    return dict(name='%s-%s%s' % (fam, MODE_NAMES[mode], '-skip' if skip else ''), family=fam, O=O, dims=dims, taps=27, Cin=64, N=232,
                mode=mode, Cin2=96 if skip else 0, rowvec=rowvec, res=True, out='both', geglu=False,
                stats=fam == 'A' and not skip and mode in (SAME, UP_HW, DOWN_HW), routes=family_routes(mode, skip))


FAMILY_CASES = [_family(f, m, s) for f in 'AB' for s in (False, True) for m in range(6) if not (s and m in UP_MODES)]


def _same(name, O, dims, taps, Cin, N, routes, rowvec=False, res=False, out='both', geglu=False):
    return dict(name=name, family=None, O=O, dims=dims, taps=taps, Cin=Cin, N=N, mode=SAME, Cin2=0, rowvec=rowvec, res=res, out=out,
                geglu=geglu, stats=False, routes=routes)


_D = lambda kernel, S=1: [Route({}, None, kernel, S)]
# kernels that take SAME launches only, and the default routes that reach a kernel without forcing
SAME_CASES = [
    # 513 objects of 128 voxels: 257 row tiles of 256 with a ragged last one; 2 / 3 column tiles walked by one workgroup
    _same('linear_ws-ncb2', 513, (4, 4, 8), 1, 32, 448, _D('linear_ws'), rowvec=True, res=True),
    _same('linear_ws-ncb3', 513, (4, 4, 8), 1, 32, 672, _D('linear_ws'), rowvec=True, res=True),
    _same('linear_ws-ncb2-geglu', 513, (4, 4, 8), 1, 32, 448, _D('linear_ws'), out='f16', geglu=True),
    _same('linear_ws-ncb3-geglu', 513, (4, 4, 8), 1, 32, 672, _D('linear_ws'), out='f16', geglu=True),
    _same('linear_deep', 5, (2, 4, 4), 1, 160, 232, [Route({'conv_few': 0}, None, 'linear_deep', 1)], res=True),
    _same('kw_4_1-default', 5, (2, 4, 4), 1, 448, 232, _D('kw_4_1'), res=True),
    _same('ws_64-default', 5, (2, 4, 4), 1, 160, 232, _D('ws_64_4_4_3'), res=True),
    _same('n16', 2, (4, 4, 16), 27, 96, 3, _D('n16'), out='ncdhw'),
    _same('small_n', 2, (4, 4, 4), 27, 64, 1, _D('small_n'), out='f32'),
    _same('small_n_tiled', 2, (8, 8, 8), 27, 32, 1, _D('small_n_tiled'), out='f32'),
    _same('geglu', 3, (4, 4, 8), 1, 64, 448,
          [Route({}, None, 'ws_64_4_4_3', 1), Route({'conv_force256': 1}, None, 'ws_256_8_4_3', 1), Route({'conv_kw_ks': 4}, None, 'kw_4_1', 1),
           Route({'conv_kw_ks': 2}, None, 'kw_2_2', 1), Route({'conv_ws': 0}, None, 'lean_64', 1)], out='f16', geglu=True),
]

CASES = FAMILY_CASES + SAME_CASES


def route_label(r):
    return (','.join('%s=%d' % kv for kv in r.options.items()) or 'default') + ('' if r.splitk is None else ' splitk=%d' % r.splitk)


def takes_workspace(case):
    """the planner's rule (plan_vol.py, VolEmitters.conv): a launch gets the split-K workspace, and splitk = -1 when the caller
    says nothing, only with a channels-last output of at most 8192 x 5376 floats, N % 4 == 0 and no GEGLU epilogue"""
    D, H, W = case['dims']
    return case['out'] != 'ncdhw' and case['O'] * D * H * W * case['N'] <= 8192 * 5376 and case['N'] % 4 == 0 and not case['geglu']


def dummy_conv_args(case, splitk):
    """the es_conv_args the planner builds for (case, splitk), with dummy pointers: for the host-only queries"""
    from echoscene_amd import hip
    a = hip.ConvArgs()
    a.a, a.w = 0x1000, 0x2000
    a.O, (a.D, a.H, a.W) = case['O'], case['dims']
    a.Cin, a.N, a.taps, a.mode = case['Cin'], case['N'], case['taps'], case['mode']
    if case['Cin2']:
        a.a2, a.w2, a.Cin2 = 0x1100, 0x2100, case['Cin2']
    a.bias = 0x5000
    if case['rowvec']:
        a.rowvec, a.rowvec_ld = 0x9000, case['N']
    a.res = 0xa000 if case['res'] else None
    a.out_f32 = 0x3000 if case['out'] in ('both', 'f32', 'ncdhw') else None
    a.out_f16 = 0x4000 if case['out'] in ('both', 'f16') else None
    a.out_ld = -1 if case['out'] == 'ncdhw' else (case['N'] // 2 if case['geglu'] else case['N'])
    a.epilogue = hip.EPI_GEGLU if case['geglu'] else hip.EPI_NONE
    if takes_workspace(case):
        a.workspace, a.splitk = 0x6000, -1 if splitk is None else splitk
    return a
