"""The GroupNorm / attention / small-kernel matrix of the volume path: the cases, and for each the route the launch rule gives it
(es_groupnorm_route_of, es_attention_route_of).  Shared by tests/test_side_matrix_cpu.py (the routes and their coverage, no GPU),
tests/test_hip_groupnorm_matrix.py and tests/test_hip_attention_matrix.py (the same launches run, against fp64).  A plain module: no
fixtures, no test.

GroupNorm case: name, O, V, C1, C2 (second source, 0: none), groups, o_hint (Builder.o_hint; 0: none), silu (0 none, 1 SiLU, 2 GELU),
fp32 (fp32 operand out, Builder.fp32), raw (the un-normalised copy is asked for), src ('pass': k_gn_partial over the sources;
'part_in': partials handed in, as a split-K conv's reduction leaves them; 'rowgroup': the producers' row-group sums), x1_f16 (the
source is an f16 tensor), eps, inputs ('varied': every (object, group) its own mean and spread; 'zero_group' / 'const_group': one group
of every object all zero / one constant; ('ratio', r): every group mean = r x spread), and `route`: the expected es_gn_route_info --
vt, ntiles, stats_src, finalize, vpb, TX; the grids follow from them (gn_grids).

The smallest shapes that reach each route, from gn_voxel_tile (start at 64, halve while vt > 8 and Oh * ceil(V / vt) < 512, Oh = the
object count of the whole / reference problem) and the vpb rule (start at 32, halve while > 8 and O * ceil(V / vpb) < 512, then
double while < 1024 and O * ceil(V / vpb) > 16384); TX = the number of 8-channel chunks rounded up to a power of two, at most 32.

Attention case: name, B, heads, Ntok, dhead, fp32, families (the input families run on it) and the expected kernel name, DP, rows
per workgroup and grid."""

# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------
GN_SOURCES = ('pass', 'part_in', 'rowgroup')          # es_gn_route_info.stats_src indexes it


def _gn(name, O, V, C1, route, C2=0, groups=32, o_hint=0, silu=1, fp32=False, raw=False, src='pass', x1_f16=False, eps=1e-5,
        inputs='varied'):
    vt, ntiles, finalize, vpb, TX = route
    return dict(name=name, O=O, V=V, C1=C1, C2=C2, groups=groups, o_hint=o_hint, silu=silu, fp32=fp32, raw=raw, src=src, x1_f16=x1_f16,
                eps=eps, inputs=inputs, route=dict(vt=vt, ntiles=ntiles, stats_src=src, finalize=finalize, vpb=vpb, TX=TX))


# route = (vt, ntiles, finalize, vpb, TX)
GN_CASES = [
    # ---- the voxel tile of the statistics pass (k_gn_partial): 64 / 32 / 16 take the four-loads-in-flight branch on full tiles
    _gn('vt64-full', 2, 512, 96, (64, 8, 0, 8, 16), o_hint=64, raw=True),
    _gn('vt64-ragged8', 2, 520, 64, (64, 9, 0, 8, 8), o_hint=64, silu=0),
    _gn('vt32', 2, 512, 128, (32, 16, 0, 8, 16), o_hint=32, silu=2),
    _gn('vt16', 2, 512, 256, (16, 32, 0, 8, 32), o_hint=16),
    _gn('vt8-64tiles', 2, 512, 64, (8, 64, 0, 8, 8), eps=1e-6),
    _gn('v100-last4', 2, 100, 64, (8, 13, 0, 8, 8), silu=2, raw=True),
    _gn('v3', 2, 3, 64, (8, 1, 0, 8, 8)),
    _gn('rows-v1-c384', 45, 1, 384, (8, 1, 0, 8, 32), fp32=True),
    _gn('rows-v1-c384-f16', 45, 1, 384, (8, 1, 0, 8, 32), silu=0),
    _gn('refshard-4', 2, 512, 64, (8, 64, 0, 8, 8), o_hint=-4, silu=0),
    # ---- the in-apply reduction of the tile list (gn_reduce_stats): 256 / groups slices of it per group
    _gn('reduce-16deep-128tiles', 1, 1024, 64, (8, 128, 0, 8, 8)),
    _gn('reduce-4deep-100tiles', 1, 800, 64, (8, 100, 0, 8, 8), silu=0),
    _gn('reduce-tail-5tiles', 1, 40, 64, (8, 5, 0, 8, 8)),
    _gn('groups30-c240', 2, 100, 240, (8, 13, 0, 8, 32), groups=30),
    _gn('groups64-c128', 2, 100, 128, (8, 13, 0, 8, 16), groups=64, silu=2, fp32=True),
    _gn('groups2-c8', 2, 100, 8, (8, 13, 0, 8, 1), groups=2),
    # ---- k_gn_finalize (more than 128 tiles), alone and behind partials handed in
    _gn('finalize-130tiles', 1, 1040, 64, (8, 130, 1, 8, 8)),
    _gn('finalize-130tiles-part_in', 1, 1040, 64, (8, 130, 1, 8, 8), src='part_in'),
    _gn('part_in-64tiles', 2, 512, 64, (8, 64, 0, 8, 8), src='part_in', silu=0),
    # ---- the apply pass: TX by width, the channel loop, voxels per block
    _gn('tx2-c16', 2, 100, 16, (8, 13, 0, 8, 2), groups=4, silu=0),
    _gn('tx4-c24', 2, 100, 24, (8, 13, 0, 8, 4), groups=3, fp32=True, raw=True),
    _gn('tx16-c128', 2, 100, 128, (8, 13, 0, 8, 16)),
    _gn('tx32-c256', 2, 100, 256, (8, 13, 0, 8, 32), silu=0, fp32=True),
    _gn('loop-c448', 2, 100, 448, (8, 13, 0, 8, 32), raw=True),
    _gn('loop-c2048', 2, 20, 2048, (8, 3, 0, 8, 32), groups=64, silu=2),
    _gn('vpb16', 8, 1024, 8, (16, 64, 0, 16, 1), groups=2),
    _gn('vpb32', 16, 1024, 8, (32, 32, 0, 32, 1), groups=2, silu=0),
    _gn('vpb64-64cubed', 3, 64 ** 3, 8, (64, 4096, 1, 64, 1), groups=2),
    # ---- two sources
    _gn('two-sources-40-56-gs3', 2, 100, 40, (8, 13, 0, 8, 16), C2=56, raw=True),
    _gn('two-sources-128-64', 2, 100, 128, (8, 13, 0, 8, 32), C2=64, silu=0),
    _gn('two-sources-fp32', 2, 100, 64, (8, 13, 0, 8, 16), C2=32, fp32=True, silu=1, raw=True),
    # ---- statistics from the producers' row-group sums (V % 64 == 0): an f16 source, two fp32 sources
    _gn('rowgroup-x1-f16', 2, 128, 64, (8, 16, 0, 8, 8), src='rowgroup', x1_f16=True),
    _gn('rowgroup-two-fp32', 2, 128, 64, (8, 16, 0, 8, 16), C2=32, src='rowgroup', raw=True, silu=0),
    # ---- degenerate groups and the cancellation in E[x^2] - mean^2
    _gn('zero-group', 2, 100, 64, (8, 13, 0, 8, 8), inputs='zero_group', silu=0),
    _gn('const-group', 2, 100, 96, (8, 13, 0, 8, 16), inputs='const_group', silu=0),
    _gn('ratio-0', 2, 100, 64, (8, 13, 0, 8, 8), inputs=('ratio', 0), silu=0),
    _gn('ratio-8', 2, 100, 64, (8, 13, 0, 8, 8), inputs=('ratio', 8), silu=0),
    _gn('ratio-64', 2, 100, 64, (8, 13, 0, 8, 8), inputs=('ratio', 64), silu=0),
]

# the launches whose bits must equal another launch's: a shard under o_hint = the matching objects of the whole problem (O = o_hint)
GN_SHARD_CASES = ('vt64-full', 'vt64-ragged8', 'vt32', 'vt16')

# every value of every route field the matrix must reach (test_side_matrix_cpu)
GN_FIELD_VALUES = dict(vt=(8, 16, 32, 64), stats_src=GN_SOURCES, finalize=(0, 1), vpb=(8, 16, 32, 64), TX=(1, 2, 4, 8, 16, 32))


def gn_grids(case):
    """the grids of the launches of a case, from its route: k_gn_partial, k_gn_finalize / k_gn_finalize_rg, k_gn_apply ((0, 0): not run)"""
    r, O = case['route'], case['O']
    partial = (r['ntiles'], O) if r['stats_src'] == 'pass' else (0, 0)
    fin = (case['groups'], O) if (r['finalize'] or r['stats_src'] == 'rowgroup') else (0, 0)
    return dict(partial=partial, finalize=fin, apply=((case['V'] + r['vpb'] - 1) // r['vpb'], O))


def gn_features(case):
    """the branches inside the kernels that a case reaches, by name: derived from the ROUTE (what the query answered) and the shape"""
    r, V, C, G = case['route'], case['V'], case['C1'] + case['C2'], case['groups']
    f = set()
    if r['stats_src'] == 'pass':
        last = V - (r['ntiles'] - 1) * r['vt']
        if r['vt'] % 16 == 0 and r['ntiles'] > (1 if last < r['vt'] else 0):
            f.add('partial:four-in-flight')
        if r['vt'] % 16 or last < r['vt']:
            f.add('partial:generic')
        if last < r['vt']:
            f.add('partial:ragged')
        if last < 4:
            f.add('partial:idle-voxel-rows')
        if C > 256:
            f.add('partial:channel-loop')
    if r['stats_src'] != 'rowgroup' and not r['finalize']:
        nsl, t = 256 // G, 0                        # slice 0 of the tile list
        if t + 15 * nsl < r['ntiles']:
            f.add('reduce:16-deep')
            while t + 15 * nsl < r['ntiles']:
                t += 16 * nsl
        if t + 3 * nsl < r['ntiles']:
            f.add('reduce:4-deep')
            while t + 3 * nsl < r['ntiles']:
                t += 4 * nsl
        if t < r['ntiles']:
            f.add('reduce:tail')
        if nsl * G < 256:
            f.add('reduce:idle-threads')
    if r['finalize']:
        f.add('finalize:part_in' if r['stats_src'] == 'part_in' else 'finalize:own-partials')
    if C > 256:
        f.add('apply:channel-loop')
    if case['C2']:
        f.add('two-sources')
        if case['C1'] % (C // G):
            f.add('two-sources:boundary-inside-a-group')
    if V == 1:
        f.add('rows-use')
    f.add('silu:%d' % case['silu'])
    f.add('out:fp32' if case['fp32'] else 'out:f16')
    f.add('raw:yes' if case['raw'] else 'raw:no')
    if case['x1_f16']:
        f.add('x1-f16')
    if case['src'] == 'rowgroup' and case['C2']:
        f.add('rowgroup:two-sources')
    if G != 32:
        f.add('groups:%d' % G)
    if case['o_hint'] < 0:
        f.add('o_hint:reference-shard')
    if case['o_hint'] > case['O']:
        f.add('o_hint:whole-problem')
    return f


GN_FEATURES = ('partial:four-in-flight', 'partial:generic', 'partial:ragged', 'partial:idle-voxel-rows', 'partial:channel-loop',
               'reduce:16-deep', 'reduce:4-deep', 'reduce:tail', 'reduce:idle-threads', 'finalize:part_in', 'finalize:own-partials',
               'apply:channel-loop', 'two-sources', 'two-sources:boundary-inside-a-group', 'rows-use', 'silu:0', 'silu:1', 'silu:2',
               'out:fp32', 'out:f16', 'raw:yes', 'raw:no', 'x1-f16', 'rowgroup:two-sources', 'groups:2', 'groups:3', 'groups:4', 'groups:30', 'groups:64',
               'o_hint:reference-shard', 'o_hint:whole-problem')

# (mean, spread) of an (object, group): means from +-{0, 0.5, 3}, spreads from {0.05, 1, 20}.  The spread goes by (g + o) % 3, so that
# neighbouring groups (g +- 1, g ^ 1) and neighbouring objects always differ in it; each spread has means of its own, so that they
# differ in the mean too.  |mean| / spread <= 3: the cancellation in E[x^2] - mean^2 has cases of its own (('ratio', r))
GN_TARGETS = (((3.0, 1.0), (-0.5, 1.0)), ((-3.0, 20.0), (0.5, 20.0)), ((0.0, 0.05), (0.0, 0.05)))


def gn_target(o, g):
    return GN_TARGETS[(g + o) % 3][((g + o) // 3) % 2]


def dummy_gn_args(case):
    """the es_gn_args the planner builds for a case, with dummy pointers: for the host-only query"""
    from echoscene_amd import hip
    a = hip.GNArgs()
    a.x1, a.C1 = 0x1000, case['C1']
    if case['C2']:
        a.x2, a.C2 = 0x2000, case['C2']
    a.O, a.V, a.groups, a.eps = case['O'], case['V'], case['groups'], case['eps']
    a.gamma, a.beta, a.silu, a.stats, a.y_f16 = 0x3000, 0x4000, case['silu'], 0x5000, 0x6000
    a.raw_f16 = 0x7000 if case['raw'] else None
    a.O_hint, a.y_is_f32, a.x1_is_f16 = case['o_hint'], int(case['fp32']), int(case['x1_f16'])
    if case['src'] == 'rowgroup':
        a.stats1 = 0x8000
        a.stats2 = 0x9000 if case['C2'] else None
    if case['src'] == 'part_in':
        a.part_in = 0xa000
    return a


def gn_route_of(L, a):
    """es_groupnorm_route_of(a) as the dict a case's `route` is compared with, + the grids; None when the arguments are refused"""
    import ctypes as C
    from echoscene_amd import hip
    i = hip.GNRouteInfo()
    if L.es_groupnorm_route_of(C.byref(a), C.byref(i)) != 0:
        return None
    return dict(vt=i.vt, ntiles=i.ntiles, stats_src=GN_SOURCES[i.stats_src], finalize=i.finalize, vpb=i.vpb, TX=i.TX), \
        dict(partial=(i.partial_gx, i.partial_gy), finalize=(i.finalize_gx, i.finalize_gy), apply=(i.apply_gx, i.apply_gy)), i.fin_offset


# ---- attention ----------------------------------------------------------------------------------------------------------------------
ATTN_F16_KERNELS = tuple('attention_%d_4_%d' % k for k in ((32, 1), (32, 2), (64, 1), (64, 2), (96, 1), (96, 2), (256, 1)))
ATTN_F32_KERNELS = ('attention_f32m_64', 'attention_f32m_96', 'attention_f32_64', 'attention_f32_96')
ATTN_FAMILIES = ('normal', 'first_tile_max', 'last_tile_max', 'peaked', 'equal_keys')
ALL_FAMILIES = ATTN_FAMILIES


def _at(B, heads, Ntok, dhead, kernel, fp32=False, families=('normal',)):
    if fp32:
        rows, DP = 64, 64 if dhead <= 64 else 96
    else:
        DP, _, nrt = (int(t) for t in kernel.split('_')[1:])
        rows = 64 * nrt
    return dict(name='%s%dx%dx%dx%d' % ('f32-' if fp32 else '', B, heads, Ntok, dhead), B=B, heads=heads, Ntok=Ntok, dhead=dhead, fp32=fp32,
                families=families, kernel=kernel, DP=DP, rows=rows, grid=((Ntok + rows - 1) // rows, B * heads))


ATTN_CASES = [
    _at(2, 3, 100, 8, 'attention_32_4_1', families=ALL_FAMILIES),          # ragged, 64-row workgroups: 2 x 6 of them
    _at(1, 1, 1, 4, 'attention_32_4_1'),                                     # one token: the output is V
    _at(1, 2, 3, 12, 'attention_32_4_1'),
    _at(1, 1, 63, 32, 'attention_32_4_1'),
    _at(1, 1, 64, 32, 'attention_32_4_1'),
    _at(1, 1, 65, 20, 'attention_32_4_1'),                                   # one key in the second tile
    _at(1, 3, 520, 20, 'attention_32_4_2', families=ALL_FAMILIES),          # ragged, 128-row workgroups: 5 x 3
    _at(2, 1, 70, 36, 'attention_64_4_1', families=ALL_FAMILIES),
    _at(1, 2, 576, 56, 'attention_64_4_2'),
    _at(1, 2, 256, 84, 'attention_96_4_1'),
    _at(1, 1, 530, 40, 'attention_64_4_2'),                                  # ... and these two instantiations with a ragged last key tile
    _at(1, 2, 100, 72, 'attention_96_4_1'),
    _at(1, 1, 520, 68, 'attention_96_4_2', families=ALL_FAMILIES),
    _at(1, 1, 130, 100, 'attention_256_4_1', families=ALL_FAMILIES),        # 3 workgroups
    _at(1, 1, 200, 256, 'attention_256_4_1'),
    _at(1, 1, 520, 128, 'attention_256_4_1', families=('normal', 'last_tile_max')),      # 9 workgroups
    _at(1, 1, 1030, 8, 'attention_32_4_2'),                                  # 9 workgroups of 128 rows
    _at(1, 17, 40, 8, 'attention_32_4_1'),                                   # 17 workgroups: the XCD remap with a remainder of 1
    # ---- es_attention_f32: the matrix-instruction kernels (dhead % 4 == 0) and the scalar ones
    _at(2, 2, 65, 8, 'attention_f32m_64', fp32=True),
    _at(1, 2, 200, 64, 'attention_f32m_64', fp32=True, families=('normal', 'peaked')),
    _at(1, 3, 65, 84, 'attention_f32m_96', fp32=True),
    _at(1, 2, 1, 84, 'attention_f32m_96', fp32=True),
    _at(2, 2, 65, 6, 'attention_f32_64', fp32=True),
    _at(1, 2, 1, 6, 'attention_f32_64', fp32=True),
    _at(1, 2, 200, 70, 'attention_f32_96', fp32=True, families=('normal', 'peaked')),
]


def dummy_attn_args(case):
    from echoscene_amd import hip
    a = hip.AttnArgs()
    a.qkv, a.out_f16 = 0x1000, 0x2000
    a.B, a.Ntok, a.heads, a.dhead = case['B'], case['Ntok'], case['heads'], case['dhead']
    a.scale = float(case['dhead']) ** -0.5
    return a


def attn_route_of(L, a, fp32):
    import ctypes as C
    from echoscene_amd import hip
    i = hip.AttnRouteInfo()
    if L.es_attention_route_of(C.byref(a), int(fp32), C.byref(i)) != 0:
        return None
    return dict(kernel=i.kernel.decode(), DP=i.DP, rows=i.rows, grid=(i.grid_x, i.grid_y), block=i.block, lds=i.lds)


def xcd_order(nwg):
    """the order in which k_attention's workgroups take (batch * head, row tile) pairs: hardware workgroup id b -> logical id"""
    xq, xr = nwg >> 3, nwg & 7
    return [(x * (xq + 1) if x < xr else xr * (xq + 1) + (x - xr) * xq) + (b >> 3) for b in range(nwg) for x in (b & 7,)]


# ---- the small kernels --------------------------------------------------------------------------------------------------------------
TOCL_CASES = [dict(name='tocl-c%d-pad%d-%s' % (c, cpad, 'f32' if f32 else 'f16'), O=2, C=c, V=100, Cpad=cpad, fp32=f32)
              for c in (1, 3, 5, 8) for cpad in (8, 32) for f32 in (False, True)]
GEGLU_CASES = [dict(name='geglu-%s' % ('f32' if f32 else 'f16'), M=50, C4=c4, fp32=f32) for f32, c4 in ((False, 64), (True, 64), (True, 36))]
SPLIT_CASES = [dict(name='split3-%dx%d' % mc, M=mc[0], C=mc[1]) for mc in ((37, 24), (3000, 64))]
SMALL_VARIANTS = {'tocl': {(c, cpad, f32) for c in (1, 3, 5, 8) for cpad in (8, 32) for f32 in (False, True)},
                  'geglu': {False, True}, 'split': {'split3'}}

