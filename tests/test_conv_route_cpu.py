"""CPU-only: the routing rule of es_conv_mfma_f16, pinned.  tests/golden/conv_routes.npz holds the answers of the three host-only
queries (es_conv_emits_gn_stats, es_conv_emits_gn_part, es_conv_split_of) over a grid of es_conv_args -- 1 to 32 objects, whole
problems, canonical shards and hinted shards, every level of the shape UNet and the VQ-VAE with their real channel pairs, 3x3x3 and
1x1, fused skips, the GEGLU epilogue, explicit and automatic splits, with and without a workspace, the planner's GroupNorm requests,
every conv mode, NCDHW output, launches over the 2 GiB descriptor limit, invalid arguments -- under the default route options and under
each option that a test or tool sets.  The routing decides where an fp32 sum is cut (a shard bit-equal to the unsharded run), how many
slabs a launch writes (the workspace the planner sizes) and which launch forms GroupNorm sums: a change of it must be deliberate.
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
    d = np.load(os.path.join(GOLDEN, 'conv_routes.npz'))
    cols, table, settings, want = [str(c) for c in d['cols']], d['cases'], [str(s) for s in d['settings']], d['answers']
    defaults = [kv.split('=') for kv in str(d['defaults']).strip(';').split(';')]
    assert want.shape == (len(settings), len(table), 3) and len(table) > 10000 and len(settings) == 13
    assert len(np.unique(want.reshape(-1, 3), axis=0)) >= 20, 'a degenerate table pins nothing'
    structs = [_conv_args(cols, row) for row in table]
    found = _options(L)
    assert [k for k, _ in found] == [k for k, _ in defaults], 'the route options changed: regenerate the table on purpose'
    try:
        for si, setting in enumerate(settings):
            _set(L, defaults)
            _set(L, [kv.split('=') for kv in setting.split(',') if kv])
            got = np.empty((len(structs), 3), dtype=np.int64)
            for ci, a in enumerate(structs):
                p = C.byref(a)
                got[ci] = (L.es_conv_emits_gn_stats(p), L.es_conv_emits_gn_part(p), L.es_conv_split_of(p))
            bad = np.nonzero((got != want[si]).any(axis=1))[0]
            assert len(bad) == 0, 'options "%s": %d of %d routes differ, first: %s -> %s, recorded %s' % (
                setting, len(bad), len(structs), dict(zip(cols, table[bad[0]].tolist())), got[bad[0]].tolist(), want[si, bad[0]].tolist())
    finally:
        _set(L, found)
