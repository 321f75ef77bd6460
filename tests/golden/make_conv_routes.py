"""Writes conv_routes.npz: every field of the route of es_conv_mfma_f16 (es_conv_route_of: kernel, grid, LDS bytes, split, slabs,
column tiles per workgroup, chunk size, the statistics and reduction flags, the folded route's schedule) over a grid of es_conv_args
crossed with route-option settings.  No device is needed: the query launches nothing.  tests/test_conv_route_cpu.py replays the table against the built library, so a change of the routing rule
shows as a changed entry; regenerate the file only when such a change is intended, and say so in the commit.

usage: python tests/golden/make_conv_routes.py               (against the library built in this tree)
       python tests/golden/make_conv_routes.py --check-old   (writes nothing: are the committed file's values, for its cases, still the answers?)

The file holds the case table (one row of small integers per es_conv_args, columns = COLS), the option settings, the option
values they start from and one array [setting][case] per route field (FIELDS, each in the narrowest integer type that holds it; -1 in
every field where the arguments are refused) -- no pointers, no tensors."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# one case = one row of these; the flag columns say which optional pointers are non-NULL (the queries never dereference them)
COLS = ('O', 'D', 'H', 'W', 'Cin', 'N', 'taps', 'mode', 'Cin2', 'epilogue', 'splitk', 'workspace', 'O_hint',
        'out',                 # 0: fp32 channels-last, 1: fp16 channels-last, 2: fp32 NCDHW (out_ld < 0), 3: no output at all
        'gn_stats_out', 'gn_part_out', 'gn_part_groups', 'rowvec', 'res',
        'w2')                  # 1: w2 WITHOUT a2 -- the folded weight image of an UP_HW launch

# the fields of es_conv_route_info, in its order
FIELDS = ('kernel', 'grid_x', 'grid_y', 'grid_z', 'lds', 'S', 'slabs', 'ncb', 'omax', 'epi_stats', 'stats', 'stats_pass', 'part_ok', 'reduce',
          'vt', 'fold_bal')

# route-option settings: '' = the defaults, otherwise name=value pairs set on top of the defaults
SETTINGS = ('', 'conv_few=0', 'conv_wssplit=0', 'conv_wss_target=512', 'conv_tile=128', 'conv_force256=1', 'conv_ws=0', 'conv_deep=0',
            'conv_tinysplit=0', 'conv_st_bm=64', 'conv_st_bm=128,conv_st_np=8', 'conv_kw_ks=4', 'conv_kw_ks=2')

# (Cin, N, taps, Cin2, epilogue) of the shape UNet (224 channels x (1, 2, 3)): ResBlock convs, convs fed by a fused skip, 1x1
# shortcuts, the output conv (224 -> 3, padded 16), the transformer linears (projections, qkv, GEGLU feed-forward) ...
UNET = [(224, 224, 27, 0, 0), (224, 448, 27, 0, 0), (448, 448, 27, 0, 0), (448, 672, 27, 0, 0), (672, 672, 27, 0, 0),
        (672, 672, 27, 672, 0), (672, 448, 27, 448, 0), (448, 448, 27, 448, 0), (448, 224, 27, 224, 0), (224, 224, 27, 224, 0),
        (224, 16, 27, 0, 0), (224, 3, 27, 0, 0),
        (224, 448, 1, 0, 0), (448, 672, 1, 0, 0), (672, 672, 1, 672, 0), (448, 448, 1, 224, 0),
        (448, 448, 1, 0, 0), (672, 672, 1, 0, 0), (448, 1344, 1, 0, 0), (672, 2016, 1, 0, 0),
        (448, 3584, 1, 0, 1), (672, 5376, 1, 0, 1), (1792, 448, 1, 0, 0), (2688, 672, 1, 0, 0), (1344, 672, 1, 0, 0)]
# ... and of the VQ-VAE (64 channels x (1, 2, 4)), whose last convs have N = 4 (z) and N = 1 (the decoded SDF)
VQVAE = [(64, 64, 27, 0, 0), (64, 128, 27, 0, 0), (128, 128, 27, 0, 0), (128, 256, 27, 0, 0), (256, 256, 27, 0, 0),
         (64, 4, 27, 0, 0), (64, 1, 27, 0, 0), (256, 4, 27, 0, 0), (64, 128, 1, 0, 0), (128, 256, 1, 0, 0), (256, 4, 1, 0, 0)]
OBJECTS = (1, 2, 4, 8, 16, 32)
HINTS = (0, -4, 32)
UNET_VOLS = ((16, 16, 16), (16, 8, 8), (16, 4, 4))
VQVAE_VOLS = ((16, 16, 16), (32, 32, 32), (64, 64, 64))            # 32 objects at 64^3 with Cin = 128: over 2 GiB, the chunked branch


def case(O, vol, layer, splitk=-1, workspace=1, hint=0, mode=0, out=0, gn_stats=0, gn_part=0, groups=0, rowvec=0, res=0, w2=0):
    cin, n, taps, cin2, epi = layer
    if epi and out == 0:
        out = 1                                                    # the GEGLU epilogue writes fp16 only
    return (O, vol[0], vol[1], vol[2], cin, n, taps, mode, cin2, epi, splitk, workspace, hint, out, gn_stats, gn_part, groups, rowvec, res, w2)


def cases():
    rows = []
    for layers, vols in ((UNET, UNET_VOLS), (VQVAE, VQVAE_VOLS)):
        for O, hint, vol, layer in itertools.product(OBJECTS, HINTS, vols, layers):
            for splitk, workspace in itertools.product((-1, 0, 2, 8), (1, 0)):
                rows.append(case(O, vol, layer, splitk, workspace, hint))
            # the planner's requests and the other output forms, on the automatic split with a workspace
            rows.append(case(O, vol, layer, hint=hint, gn_stats=1))
            rows.append(case(O, vol, layer, hint=hint, gn_stats=1, out=1))
            rows.append(case(O, vol, layer, hint=hint, gn_part=1, groups=32))
            rows.append(case(O, vol, layer, hint=hint, groups=32))
            rows.append(case(O, vol, layer, hint=hint, gn_stats=1, gn_part=1, groups=32))
            rows.append(case(O, vol, layer, hint=hint, out=1))
            rows.append(case(O, vol, layer, hint=hint, out=2))
            rows.append(case(O, vol, layer, hint=hint, rowvec=1))
            rows.append(case(O, vol, layer, hint=hint, res=1))
            for mode in (1, 2, 3, 4, 5):                           # every conv mode (where the mode refuses the layer the answer is -1)
                rows.append(case(O, vol, layer, hint=hint, mode=mode))
                rows.append(case(O, vol, layer, hint=hint, mode=mode, gn_stats=1))
    # more objects than any scene has: chunked launches with the canonical-shard arithmetic, and without
    for O, hint in ((1024, -4), (1024, 0), (64, 0), (256, -4)):
        rows.append(case(O, (16, 16, 16), UNET[0], hint=hint))
        rows.append(case(O, (16, 16, 16), (672, 224, 27, 0, 0), hint=hint))
        rows.append(case(O, (64, 64, 64), VQVAE[2], hint=hint, gn_stats=1))
        rows.append(case(O, (64, 64, 64), VQVAE[2], hint=hint, workspace=0))
    # invalid arguments: the answer is -1
    ok = UNET[0]
    rows.append(case(4, (16, 16, 16), (100, 224, 27, 0, 0)))       # Cin not a multiple of 32
    rows.append(case(4, (16, 16, 16), (224, 224, 9, 0, 0)))        # taps
    rows.append(case(4, (16, 16, 16), (224, 224, 27, 100, 0)))     # Cin2
    rows.append(case(4, (16, 12, 16), ok))                         # not a power of two
    rows.append(case(4, (16, 16, 16), ok, mode=9))
    rows.append(case(4, (16, 16, 16), ok, out=3))                  # no output
    rows.append(case(4, (16, 16, 16), (448, 3000, 1, 0, 1)))       # GEGLU with N % 224 != 0
    rows.append(case(4, (16, 16, 16), (448, 3584, 1, 0, 1), splitk=2))
    rows.append(case(4, (16, 16, 16), ok, out=2, res=1))           # NCDHW with a residual
    rows.append(case(4, (16, 16, 16), (224, 3, 27, 0, 0), gn_stats=1))
    rows.append(case(4, (16, 4, 2), ok, gn_stats=1))               # 32 voxels per object
    # UP_HW launches that carry their folded image (w2 without a2): the two up-sampling convs of the shape UNet (448 -> 448 at 16^3,
    # 672 -> 672 at 16x8x8, whose 384 tiles take the balanced schedule), 224 -> 224 at 16^3, and a volume whose D * H/2 * W/2 is no
    # multiple of 256 (16x4x4) -- with and without a workspace, whole problems, canonical shards and hinted shards.  Appended behind
    # the older cases, so that their indices stay what they were
    for O, hint, workspace, splitk in itertools.product(OBJECTS + (64,), HINTS, (0, 1), (-1, 0)):
        for vol, layer in (((16, 16, 16), UNET[2]), ((16, 8, 8), UNET[4]), ((16, 16, 16), UNET[0]), ((16, 4, 4), UNET[4])):
            rows.append(case(O, vol, layer, splitk, workspace, hint, mode=2, w2=1))
            rows.append(case(O, vol, layer, splitk, workspace, hint, mode=2, w2=1, gn_stats=1))
    return np.asarray(rows, dtype=np.int32)


def conv_args(hip, row):
    r = dict(zip(COLS, (int(v) for v in row)))
    a = hip.ConvArgs()
    a.a, a.w, a.bias = 0x1000, 0x2000, 0x5000
    for k in ('O', 'D', 'H', 'W', 'Cin', 'N', 'taps', 'mode', 'epilogue', 'splitk', 'O_hint', 'gn_part_groups'):
        setattr(a, k, r[k])
    if r['Cin2']:
        a.a2, a.w2, a.Cin2 = 0x1100, 0x2100, r['Cin2']
    if r['w2']:
        a.w2 = 0x2100
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


def route_options(hip):
    buf = C.create_string_buffer(1024)
    hip.lib().es_vol_options(buf, 1024)
    return buf.value.decode()


def answers(hip, table, settings):
    """[setting][case][field of FIELDS], -1 in every field where the arguments are refused; every option a setting changes is restored"""
    L = hip.lib()
    defaults = dict(kv.split('=') for kv in route_options(hip).strip(';').split(';'))
    structs = [conv_args(hip, row) for row in table]
    out = np.full((len(settings), len(structs), len(FIELDS)), -1, dtype=np.int64)
    info = hip.ConvRouteInfo()
    for si, setting in enumerate(settings):
        pairs = [kv.split('=') for kv in str(setting).split(',') if kv]
        try:
            for k, v in pairs:
                hip.check(L.es_vol_set_option(k.encode(), int(v)), 'es_vol_set_option')
            for ci, a in enumerate(structs):
                if L.es_conv_route_of(C.byref(a), C.byref(info)) == 0:
                    out[si, ci] = [getattr(info, f) for f in FIELDS]
        finally:
            for k, _ in pairs:
                hip.check(L.es_vol_set_option(k.encode(), int(defaults[k])), 'es_vol_set_option')
    return out


def narrow(v):
    """v in the smallest signed integer type that holds all of it"""
    for t in (np.int8, np.int16, np.int32):
        if np.iinfo(t).min <= v.min() and v.max() <= np.iinfo(t).max:
            return v.astype(t)
    raise ValueError('a route field beyond 32 bits')


if __name__ == '__main__':
    from echoscene_amd import hip
    table = cases()
    ans = answers(hip, table, SETTINGS)
    path = os.path.join(HERE, 'conv_routes.npz')
    if '--check-old' in sys.argv:
        # before a regeneration that only ADDS cases or fields: what the committed file holds, for the cases it holds, must be what
        # the library gives now (exit status 1 if not; nothing is written)
        old = np.load(path)
        n, w = old['cases'].shape
        assert (old['cases'] == table[:n, :w]).all() and not table[:n, w:].any() and [str(s) for s in old['settings']] == list(SETTINGS)
        moved = sum(int((ans[:, :n, FIELDS.index(str(f))] != old['f_' + str(f)]).sum()) for f in old['fields'])
        print('%d old cases x %d settings x %d fields: %d recorded values differ' % (n, len(SETTINGS), len(old['fields']), moved))
        sys.exit(int(moved != 0))
    np.savez_compressed(path, cols=np.asarray(COLS), cases=table, settings=np.asarray(SETTINGS), fields=np.asarray(FIELDS),
                        defaults=np.asarray(route_options(hip)),          # the option values every setting starts from
                        **{'f_' + f: narrow(ans[:, :, k]) for k, f in enumerate(FIELDS)})
    routes, counts = np.unique(ans.reshape(-1, len(FIELDS)), axis=0, return_counts=True)
    print('%d cases x %d settings, %d distinct routes, %d bytes; by kernel:' % (len(table), len(SETTINGS), len(routes), os.path.getsize(path)))
    for k in np.unique(ans[:, :, 0]):
        print('  %-16s %d' % ('(refused)' if k < 0 else hip.CONV_KERNELS[k], int((ans[:, :, 0] == k).sum())))
