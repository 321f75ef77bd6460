"""CPU-only: the routes of the GroupNorm / attention matrix (tests/side_matrix_cases.py).  tests/test_hip_groupnorm_matrix.py and
tests/test_hip_attention_matrix.py run every launch of that table on the GPU and mean a NAMED route by each; here the library's
host-only queries es_groupnorm_route_of / es_attention_route_of -- the rule the launchers themselves call -- answer for the same
arguments which tiles, which statistics source, which kernels and which grids a launch would take.  A change of a launch rule that
moves a case onto another route fails in the first tests; one that leaves a route without a case fails in the coverage tests.
No device compute."""
import ctypes as C

import pytest

import side_matrix_cases as sm


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


def test_every_groupnorm_case_takes_the_route_the_table_names(L):
    bad = []
    for case in sm.GN_CASES:
        got = sm.gn_route_of(L, sm.dummy_gn_args(case))
        if got is None:
            bad.append('%s: refused: %s' % (case['name'], L.es_last_error().decode()))
            continue
        route, grids, fin_off = got
        if route != case['route']:
            bad.append('%s: %s; the table says %s' % (case['name'], route, case['route']))
        if grids != sm.gn_grids(case):
            bad.append('%s: grids %s; the route implies %s' % (case['name'], grids, sm.gn_grids(case)))
        # where the final statistics go: behind the partials of the caller's scratch, or at its front when the partials are the producer's
        want = -1
        if route['stats_src'] == 'rowgroup' or (route['finalize'] and route['stats_src'] == 'part_in'):
            want = 0
        elif route['finalize']:
            want = case['O'] * route['ntiles'] * case['groups'] * 2
        if fin_off != want:
            bad.append('%s: final statistics at %d floats, expected %d' % (case['name'], fin_off, want))
        # the scratch the planner allocates (plan_vol.groupnorm) holds whatever the route writes into it
        need = case['O'] * ((case['V'] + 7) // 8) * case['groups'] * 2 + case['O'] * case['groups'] * 2
        used = (case['O'] * route['ntiles'] * case['groups'] * 2 if route['stats_src'] == 'pass' else 0)
        if fin_off >= 0:
            used = max(used, fin_off + case['O'] * case['groups'] * 2)
        if used > need:
            bad.append('%s: the route writes %d floats of a scratch of %d' % (case['name'], used, need))
    assert len(sm.GN_CASES) >= 35 and not bad, '\n'.join(bad)


def test_the_groupnorm_matrix_reaches_every_value_of_every_route_field():
    for field, values in sm.GN_FIELD_VALUES.items():
        have = {c['route'][field] for c in sm.GN_CASES}
        assert have == set(values), '%s: reached %s, the rule can give %s' % (field, sorted(have, key=str), values)
    reached = set().union(*(sm.gn_features(c) for c in sm.GN_CASES))
    assert reached == set(sm.GN_FEATURES), 'not reached / unknown: %s' % sorted(reached ^ set(sm.GN_FEATURES))
    # the finalize route with partials handed in, and every activation with both output types
    assert {(c['silu'], c['fp32']) for c in sm.GN_CASES} == {(s, f) for s in (0, 1, 2) for f in (False, True)}
    assert {c['inputs'] if isinstance(c['inputs'], str) else c['inputs'][1] for c in sm.GN_CASES} == {'varied', 'zero_group', 'const_group', 0, 8, 64}
    names = [c['name'] for c in sm.GN_CASES]
    assert len(set(names)) == len(names) and set(sm.GN_SHARD_CASES) <= set(names)
    for n in sm.GN_SHARD_CASES:
        c = next(c for c in sm.GN_CASES if c['name'] == n)
        assert c['o_hint'] > c['O'] and c['src'] == 'pass'


def test_the_tx_rule_gives_a_power_of_two_that_covers_the_chunks(L):
    """TX of es_gn_route_info for every legal width: the smallest power of two >= C / 8, at most 32"""
    case = dict(sm.GN_CASES[0])
    for Cc in range(8, 2049, 8):
        a = sm.dummy_gn_args(dict(case, C1=Cc, C2=0, groups=1))
        tx = sm.gn_route_of(L, a)[0]['TX']
        assert tx in (1, 2, 4, 8, 16, 32) and (tx >= Cc // 8 or tx == 32) and (tx == 1 or tx // 2 < Cc // 8), (Cc, tx)


def test_neighbouring_groups_and_objects_get_different_statistics():
    """the inputs of the GroupNorm matrix: a kernel that took the statistics of group g ^ 1, g +- 1 or of the next object is off by
    at least 10 % in the mean (of the larger spread) and in the spread"""
    flat = [t for row in sm.GN_TARGETS for t in row]
    assert {abs(m) for m, _ in flat} == {0.0, 0.5, 3.0} and {m for m, _ in flat} >= {-3.0, 3.0, -0.5, 0.5} and {s for _, s in flat} == {0.05, 1.0, 20.0}
    assert all(abs(m) / s <= 3 for m, s in flat)
    for o in range(64):
        for g in range(64):
            m0, s0 = sm.gn_target(o, g)
            for o1, g1 in ((o, g + 1), (o, g ^ 1), (o + 1, g)):
                m1, s1 = sm.gn_target(o1, g1)
                assert abs(m0 - m1) >= 0.1 * max(abs(m0), abs(m1), 0.5) and abs(s0 - s1) >= 0.1 * max(s0, s1), (o, g, o1, g1)


def test_every_attention_case_takes_the_kernel_the_table_names(L):
    bad = []
    for case in sm.ATTN_CASES:
        got = sm.attn_route_of(L, sm.dummy_attn_args(case), case['fp32'])
        if got is None:
            bad.append('%s: refused: %s' % (case['name'], L.es_last_error().decode()))
            continue
        want = {k: case[k] for k in ('kernel', 'DP', 'rows', 'grid')}
        if {k: got[k] for k in want} != want:
            bad.append('%s: %s; the table says %s' % (case['name'], got, want))
        scalar = case['fp32'] and case['dhead'] % 4 != 0
        if got['block'] != (64 if scalar else 256):
            bad.append('%s: %d threads' % (case['name'], got['block']))
        # dynamic LDS: only the fp32 matrix-instruction kernels (K and V tiles of 64 x (DP + 4) floats, 4 x 16 x 68 of probabilities)
        lds = (2 * 64 * (got['DP'] + 4) + 4 * 16 * 68) * 4 if case['fp32'] and not scalar else 0
        if got['lds'] != lds:
            bad.append('%s: %d bytes of dynamic LDS, expected %d' % (case['name'], got['lds'], lds))
    assert not bad, '\n'.join(bad)


def test_the_attention_matrix_reaches_every_instantiation_and_every_family():
    f16 = [c for c in sm.ATTN_CASES if not c['fp32']]
    f32 = [c for c in sm.ATTN_CASES if c['fp32']]
    assert {c['kernel'] for c in f16} == set(sm.ATTN_F16_KERNELS) and len(sm.ATTN_F16_KERNELS) == 7
    assert {c['kernel'] for c in f32} == set(sm.ATTN_F32_KERNELS)
    names = [c['name'] for c in sm.ATTN_CASES]
    assert len(set(names)) == len(names)
    # every family on a ragged 128-row case, a ragged 64-row case and the DP = 256 kernel
    for fam in sm.ATTN_FAMILIES:
        on = [c for c in f16 if fam in c['families']]
        assert any(c['rows'] == 128 and c['Ntok'] % 64 for c in on) and any(c['rows'] == 64 and c['Ntok'] % 64 for c in on), fam
    assert all(set(sm.ATTN_FAMILIES) <= set(c['families']) for c in f16 if c['name'] in ('1x1x130x100',))
    # every instantiation meets a ragged last key tile
    assert {c['kernel'] for c in f16 if c['Ntok'] % 64} == set(sm.ATTN_F16_KERNELS)
    # sequence lengths: one token, fewer than a tile, exactly one tile, one key more; fp32: 1, 65 and 200 tokens with several heads
    assert {1, 3, 63, 64, 65} <= {c['Ntok'] for c in f16}
    assert {c['Ntok'] for c in f32} == {1, 65, 200} and all(c['heads'] > 1 for c in f32)
    assert {c['dhead'] for c in f32} == {8, 64, 84, 6, 70}
    # workgroup counts with every kind of remainder the XCD remap distinguishes, 1 / 3 / 9 / 17 among them; the remap is a bijection
    counts = {c['grid'][0] * c['grid'][1] for c in f16}
    assert {1, 3, 9, 17} <= counts
    for n in sorted(counts):
        assert sorted(sm.xcd_order(n)) == list(range(n)), n


def test_the_small_kernel_tables_hold_every_listed_variant():
    assert {(c['C'], c['Cpad'], c['fp32']) for c in sm.TOCL_CASES} == sm.SMALL_VARIANTS['tocl'] and all(c['V'] == 100 for c in sm.TOCL_CASES)
    assert {c['fp32'] for c in sm.GEGLU_CASES} == sm.SMALL_VARIANTS['geglu']
    assert len(sm.SPLIT_CASES) >= 1 and all(c['C'] % 4 == 0 for c in sm.SPLIT_CASES)


def test_the_queries_refuse_what_the_launchers_refuse(L):
    from echoscene_amd import hip
    base = next(c for c in sm.GN_CASES if c['name'] == 'vt8-64tiles')
    gi = hip.GNRouteInfo()
    gi.vt = -7
    for change, text in ((dict(groups=5), b'groups'), (dict(C1=36, C2=28), b'multiples of 8'), (dict(groups=128, C1=128), b'groups'),
                         (dict(C1=2056), b'C=2056'), (dict(x1_f16=True), b'f16 source'), (dict(src='part_in', C2=64), b'part_in')):
        a = sm.dummy_gn_args(dict(base, **change))
        assert L.es_groupnorm_route_of(C.byref(a), C.byref(gi)) == -1 and text in L.es_last_error() and gi.vt == -7, change
    a = sm.dummy_gn_args(base)
    a.stats = None
    assert L.es_groupnorm_route_of(C.byref(a), C.byref(gi)) == -1 and b'scratch' in L.es_last_error()
    ai = hip.AttnRouteInfo()
    for fp32, change, text in ((0, dict(dhead=6), b'multiple of 4'), (0, dict(dhead=260), b'dhead=260'), (1, dict(dhead=100), b'<= 96'),
                               (0, dict(Ntok=0), b'Ntok=0')):
        a = sm.dummy_attn_args(dict(sm.ATTN_CASES[0], **change))
        assert L.es_attention_route_of(C.byref(a), fp32, C.byref(ai)) == -1 and text in L.es_last_error(), change
    a = sm.dummy_attn_args(sm.ATTN_CASES[0])
    a.scale = 0.0
    assert L.es_attention_route_of(C.byref(a), 0, C.byref(ai)) == -1 and b'scale' in L.es_last_error()
    assert L.es_attention_route_of(C.byref(a), 1, C.byref(ai)) == 0          # (the fp32 kernels scale the queries: any scale)


def test_the_rowgroup_route_follows_the_gn_rg_option_except_for_an_f16_source(L):
    """gn_rg = 0 sends fp32 sources with row-group sums back to the pass over the tensor; an f16 source has no other route"""
    from test_conv_route_cpu import _options, _set
    found = _options(L)
    two = next(c for c in sm.GN_CASES if c['name'] == 'rowgroup-two-fp32')
    f16 = next(c for c in sm.GN_CASES if c['name'] == 'rowgroup-x1-f16')
    try:
        _set(L, [('gn_rg', 0)])
        assert sm.gn_route_of(L, sm.dummy_gn_args(two))[0]['stats_src'] == 'pass'
        assert sm.gn_route_of(L, sm.dummy_gn_args(f16))[0]['stats_src'] == 'rowgroup'
    finally:
        _set(L, found)
    assert sm.gn_route_of(L, sm.dummy_gn_args(two))[0]['stats_src'] == 'rowgroup'
    # not a multiple of 64 voxels: no row groups to reduce
    assert sm.gn_route_of(L, sm.dummy_gn_args(dict(two, V=100)))[0]['stats_src'] == 'pass'
