"""CPU-only: the routing rule of es_conv_mfma_f16, pinned.  tests/golden/conv_routes.npz holds every field of the route
(es_conv_route_of: kernel, grid, LDS bytes, split, slabs, column tiles per workgroup, chunk size, the statistics and reduction flags,
the folded route's schedule) over a grid of es_conv_args -- 1 to 32 objects, whole
problems, canonical shards and hinted shards, every level of the shape UNet and the VQ-VAE with their real channel pairs, 3x3x3 and
1x1, fused skips, the GEGLU epilogue, explicit and automatic splits, with and without a workspace, the planner's GroupNorm requests,
every conv mode, NCDHW output, launches over the 2 GiB descriptor limit, UP_HW launches with their folded weight image, invalid
arguments -- under the default route options and under
each option that a test or tool sets.  The routing decides where an fp32 sum is cut (a shard bit-equal to the unsharded run), how many
slabs a launch writes (the workspace the planner sizes), which launch forms GroupNorm sums and the grid every kernel runs on (a
wrong one would first show as a GPU fault): a change of it must be deliberate.
tests/golden/make_conv_routes.py wrote the table and writes it again when the rule is changed on purpose.  No device compute here."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


def _options(L):
    buf = C.create_string_buffer(1024)
    L.es_vol_options(buf, 1024)
    return [kv.split('=') for kv in buf.value.decode().strip(';').split(';')]


def _set(L, pairs):
    from echoscene_amd import hip
    for k, v in pairs:
        hip.check(L.es_vol_set_option(k.encode(), int(v)), 'es_vol_set_option')


def _conv_args(cols, row):
    from echoscene_amd import hip
    r = dict(zip(cols, (int(v) for v in row)))
    a = hip.ConvArgs()
    a.a, a.w, a.bias = 0x1000, 0x2000, 0x5000                      # (never dereferenced by the queries)
    for k in ('O', 'D', 'H', 'W', 'Cin', 'N', 'taps', 'mode', 'epilogue', 'splitk', 'O_hint', 'gn_part_groups'):
        setattr(a, k, r[k])
    if r['Cin2']:
        a.a2, a.w2, a.Cin2 = 0x1100, 0x2100, r['Cin2']
    if r.get('w2'):
        a.w2 = 0x2100                                              # (w2 without a2: the folded image of an UP_HW launch)
    a.out_ld = -1 if r['out'] == 2 else (r['N'] // 2 if r['epilogue'] else r['N'])
    a.out_f32 = 0x3000 if r['out'] in (0, 2) else None
    a.out_f16 = 0x4000 if r['out'] == 1 else None
    a.workspace = 0x6000 if r['workspace'] else None
    a.gn_stats_out = 0x7000 if r['gn_stats_out'] else None
    a.gn_part_out = 0x8000 if r['gn_part_out'] else None
    if r['rowvec']:
        a.rowvec, a.rowvec_ld = 0x9000, r['N']
    a.res = 0xa000 if r['res'] else None
    return a


def test_conv_routes_equal_the_recorded_table(L):
    from echoscene_amd import hip
    d = np.load(os.path.join(GOLDEN, 'conv_routes.npz'))
    cols, table, settings = [str(c) for c in d['cols']], d['cases'], [str(s) for s in d['settings']]
    fields = [str(f) for f in d['fields']]
    assert fields == [f for f, _ in hip.ConvRouteInfo._fields_], 'es_conv_route_info changed: regenerate the table on purpose'
    want = np.stack([d['f_' + f].astype(np.int64) for f in fields], axis=-1)             # [setting][case][field]
    defaults = [kv.split('=') for kv in str(d['defaults']).strip(';').split(';')]
    assert want.shape == (len(settings), len(table), len(fields)) and len(table) > 10000 and len(settings) == 13
    old3 = [fields.index(f) for f in ('epi_stats', 'part_ok', 'slabs')]
    assert len(np.unique(want[:, :, old3].reshape(-1, 3), axis=0)) >= 20, 'a degenerate table pins nothing'
    kernel, fold_bal = want[:, :, fields.index('kernel')], want[:, :, fields.index('fold_bal')]
    assert (kernel == hip.CONV_KERNELS.index('ws_256_up_fold')).any() and (fold_bal == 1).any(), 'the folded route is not in the table'
    structs = [_conv_args(cols, row) for row in table]
    found = _options(L)
    assert [k for k, _ in found] == [k for k, _ in defaults], 'the route options changed: regenerate the table on purpose'
    info = hip.ConvRouteInfo()
    try:
        for si, setting in enumerate(settings):
            _set(L, defaults)
            _set(L, [kv.split('=') for kv in setting.split(',') if kv])
            got = np.full((len(structs), len(fields)), -1, dtype=np.int64)               # (refused arguments: -1 in every field)
            for ci, a in enumerate(structs):
                if L.es_conv_route_of(C.byref(a), C.byref(info)) == 0:
                    got[ci] = [getattr(info, f) for f in fields]
            bad = np.nonzero((got != want[si]).any(axis=1))[0]
            assert len(bad) == 0, 'options "%s": %d of %d routes differ, first: %s -> %s, recorded %s' % (
                setting, len(bad), len(structs), dict(zip(cols, table[bad[0]].tolist())), dict(zip(fields, got[bad[0]].tolist())),
                dict(zip(fields, want[si, bad[0]].tolist())))
    finally:
        _set(L, found)


def test_the_older_queries_read_the_same_route(L):
    """es_conv_emits_gn_stats / _gn_part / es_conv_split_of / es_conv_kernel_of / es_conv_fold_balanced are readers of the route that
    es_conv_route_of copies out: on a sample of the table each answers its field (-1 where the arguments are refused)"""
    from echoscene_amd import hip
    d = np.load(os.path.join(GOLDEN, 'conv_routes.npz'))
    cols, table = [str(c) for c in d['cols']], d['cases']
    info, name = hip.ConvRouteInfo(), C.create_string_buffer(32)
    refused = 0
    for row in table[::37]:
        a = _conv_args(cols, row)
        p = C.byref(a)
        five = (L.es_conv_emits_gn_stats(p), L.es_conv_emits_gn_part(p), L.es_conv_split_of(p), L.es_conv_kernel_of(p, name, 32),
                L.es_conv_fold_balanced(p))
        if L.es_conv_route_of(p, C.byref(info)) != 0:
            assert five == (-1,) * 5 and L.es_last_error()
            refused += 1
            continue
        assert five == (info.epi_stats, info.part_ok, info.slabs, max(info.S, 1), info.fold_bal), dict(zip(cols, row.tolist()))
        assert name.value.decode() == ('chunked' if info.omax else hip.CONV_KERNELS[info.kernel])
    assert 0 < refused < len(table[::37]) // 2
