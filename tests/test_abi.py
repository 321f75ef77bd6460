"""CPU-only checks of the C-ABI boundary: the shared library loads, exports every symbol that
include/echoscene_hip.h declares, and the host-side packers produce the documented layouts.
No device compute is called here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


def test_every_declared_symbol_is_exported(L):
    from echoscene_amd import hip
    hdr = open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read()
    declared = set(re.findall(r'\b(es_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) >= 20
    raw = C.CDLL(hip.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(raw, name), 'libechoscene_hip.so lacks %s' % name
    assert declared == set(hip.EXPORTS), 'ctypes table and header disagree: %s' % (declared ^ set(hip.EXPORTS))
    assert L.es_abi_version() == 10


def test_struct_sizes_match_header(L, tmp_path):
    """sizeof() of every ABI struct as seen by the C compiler == the ctypes mirror."""
    import subprocess
    from echoscene_amd import hip
    names = {'es_seg': hip.Seg, 'es_linear_args': hip.LinearArgs, 'es_update_args': hip.UpdateArgs,
             'es_conv_args': hip.ConvArgs, 'es_gn_args': hip.GNArgs, 'es_ln_args': hip.LNArgs,
             'es_attn_args': hip.AttnArgs, 'es_geglu_args': hip.GegluArgs, 'es_copy_args': hip.CopyArgs,
             'es_tocl_args': hip.ToClArgs, 'es_stem_args': hip.StemArgs, 'es_vq_args': hip.VQArgs,
             'es_rowsel_args': hip.RowSelArgs, 'es_conv_route_info': hip.ConvRouteInfo,
             'es_gn_route_info': hip.GNRouteInfo, 'es_attn_route_info': hip.AttnRouteInfo,
             'es_rows_route_prob': hip.RowsRouteProb, 'es_rows_route_launch': hip.RowsRouteLaunch, 'es_rows_route_info': hip.RowsRouteInfo,
             'es_op': hip.Op}
    src = '#include <stdio.h>\n#include "echoscene_hip.h"\nint main(){' + ''.join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + 'return 0;}'
    c = tmp_path / 'sz.c'
    c.write_text(src)
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    sizes = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert sizes[n] == C.sizeof(cls), '%s: C %d vs ctypes %d' % (n, sizes[n], C.sizeof(cls))


def test_route_info_layouts_match_header(L, tmp_path):
    """es_gn_route_info / es_attn_route_info / es_rows_route_info with its two member structs (es_groupnorm_route_of,
    es_attention_route_of, es_linear_rows_route_of): every field of the ctypes mirrors sits at the offset and has the size the C compiler
    gives it, and the statistics sources and the rows fall-back reasons are numbered as the header's enums"""
    import subprocess
    from echoscene_amd import hip
    structs = {'es_gn_route_info': hip.GNRouteInfo, 'es_attn_route_info': hip.AttnRouteInfo, 'es_rows_route_prob': hip.RowsRouteProb,
               'es_rows_route_launch': hip.RowsRouteLaunch, 'es_rows_route_info': hip.RowsRouteInfo}
    prints = ''.join('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (n, f[0], n, f[0], n, f[0])
                     for n, cls in structs.items() for f in cls._fields_)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "echoscene_hip.h"\nint main(){' + prints + \
          'printf("fb' + ' %d' * len(hip.ROWS_FALLBACKS) + ' %d\\n", ' + ', '.join('ES_ROWS_FB_' + f.upper() for f in hip.ROWS_FALLBACKS) + \
          ', ES_ROWS_FB_COUNT);printf("src %d %d %d\\n", ES_GN_STATS_PASS, ES_GN_STATS_PART_IN, ES_GN_STATS_ROWGROUP);return 0;}'
    c = tmp_path / 'off.c'
    c.write_text(src)
    exe = tmp_path / 'off'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    lines = [ln.split() for ln in subprocess.check_output([str(exe)]).decode().strip().split('\n')]
    got = {ln[0]: (int(ln[1]), int(ln[2])) for ln in lines[:-2]}
    n_fields = 0
    for n, cls in structs.items():
        for f in cls._fields_:
            d = getattr(cls, f[0])
            assert got['%s.%s' % (n, f[0])] == (d.offset, d.size), (n, f[0], got['%s.%s' % (n, f[0])], (d.offset, d.size))
            n_fields += 1
    assert n_fields == len(got) == 13 + 7 + 9 + 18 + 2
    assert [int(v) for v in lines[-1][1:]] == [hip.GN_STATS_SOURCES.index(s) for s in ('pass', 'part_in', 'rowgroup')]
    assert [int(v) for v in lines[-2][1:]] == list(range(len(hip.ROWS_FALLBACKS) + 1))


def test_rows_slice_choice_depends_on_k_and_n_only(L):
    """Host logic of the split-K rows launches (no device work): the default slice width is a function of (K, N) -- never of M,
    so a row's arithmetic does not depend on the batch it is in -- slices are whole multiples of the GroupNorm group, a LayerNorm /
    activation epilogue refuses a split, and es_linear_rows_slices reports the slab count the planner must allocate."""
    from echoscene_amd import hip
    assert L.es_linear_rows_auto_slices(512, 512, 16) == 8          # 32 k-blocks, 32 column tiles -> 4 slices of 8 k-blocks
    assert L.es_linear_rows_auto_slices(1024, 512, 32) == 16        # slices of 256 columns = 8 GroupNorm groups of 32
    assert L.es_linear_rows_auto_slices(512, 4096, 16) == 0         # 256 column tiles already: no split
    assert L.es_linear_rows_auto_slices(64, 512, 16) == 0           # a slice is at least 128 columns
    a = hip.LinearArgs()
    a.nseg, a.K, a.N = 1, 1536, 512
    a.seg[0].width = 1536
    got = C.c_int(0)
    for M in (1, 32, 2048):
        a.M = M
        a.kb_per_slice = L.es_linear_rows_auto_slices(a.K, a.N, 16)
        assert L.es_linear_rows_slices(C.byref(a), C.byref(got)) == 4 and got.value == 24
    a.kb_per_slice = 7
    a.seg[0].pro, a.seg[0].gs = hip.PRO_GN_SILU, 32               # groups of 32 channels = 2 k-blocks: 7 -> 8
    assert L.es_linear_rows_slices(C.byref(a), C.byref(got)) == 12 and got.value == 8
    a.kb_per_slice = 0
    assert L.es_linear_rows_slices(C.byref(a), C.byref(got)) == 1 and got.value == 96


def test_op_pointer_table_covers_every_pointer_field(L):
    """Model files relocate the device pointers of an op through es_op_pointer_offsets: the table must list exactly the c_void_p
    fields of the op's argument struct (ctypes mirror), or a saved plan would keep a stale address."""
    from echoscene_amd import hip

    def ptr_offsets(struct, base=0):
        out = []
        for name, typ in struct._fields_:
            off = base + getattr(struct, name).offset
            if typ is C.c_void_p:
                out.append(off)
            elif isinstance(typ, type) and issubclass(typ, C.Array) and issubclass(typ._type_, C.Structure):
                for k in range(typ._length_):
                    out += ptr_offsets(typ._type_, off + k * C.sizeof(typ._type_))
            elif isinstance(typ, type) and issubclass(typ, C.Structure):
                out += ptr_offsets(typ, off)
        return out

    u_off = hip.Op.u.offset
    kinds = {hip.OP_LINEAR: hip.LinearArgs, hip.OP_DDPM: hip.UpdateArgs, hip.OP_DDIM: hip.UpdateArgs, hip.OP_COPY: hip.CopyArgs,
             hip.OP_CONV: hip.ConvArgs, hip.OP_GN: hip.GNArgs, hip.OP_LN: hip.LNArgs, hip.OP_ATTN: hip.AttnArgs,
             hip.OP_GEGLU: hip.GegluArgs, hip.OP_TO_CL: hip.ToClArgs, hip.OP_STEM: hip.StemArgs, hip.OP_VQ: hip.VQArgs,
             hip.OP_ROWSEL: hip.RowSelArgs}
    buf = (C.c_size_t * 64)()
    for kind, struct in kinds.items():
        n = L.es_op_pointer_offsets(kind, buf, 64)
        assert n >= 0
        assert sorted(buf[i] for i in range(n)) == sorted(u_off + o for o in ptr_offsets(struct)), (kind, struct.__name__)
    assert L.es_op_pointer_offsets(hip.OP_FORK, buf, 64) == 0 and L.es_op_pointer_offsets(99, buf, 64) == -1


def test_pack_linear_layout(L):
    rs = np.random.RandomState(0)
    N, K = 21, 38
    W = rs.standard_normal((N, K)).astype(np.float32)
    n = L.es_pack_linear_f32_size(N, K)
    assert n == 2 * 3 * 256
    out = np.zeros(n, np.float32)
    assert L.es_pack_linear_f32(W.ctypes.data, N, K, out.ctypes.data) == 0
    o = out.reshape(2, 3, 64, 4)
    for nt in range(2):
        for kb in range(3):
            for lane in range(64):
                j, q = lane & 15, lane >> 4
                for e in range(4):
                    nn, kk = nt * 16 + j, kb * 16 + 4 * q + e
                    exp = W[nn, kk] if (nn < N and kk < K) else 0.0
                    assert o[nt, kb, lane, e] == exp


def test_holders_refuse_to_compute():
    from echoscene_amd.model.graph import GraphTripleConvNet
    net = GraphTripleConvNet(8, 4, num_layers=1, hidden_dim=8, residual=True, mlp_normalization='batch')
    with pytest.raises(RuntimeError, match='parameter container'):
        net(torch.zeros(1, 8))


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure; nothing under echoscene_amd/ or model/ may reference it."""
    bad = []
    for base in ('echoscene_amd', 'model'):
        for d, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith('.py'):
                    txt = open(os.path.join(d, f)).read()
                    if re.search(r'^\s*(from|import)\s+oracle\b', txt, re.M):
                        bad.append(os.path.join(d, f))
    assert not bad, bad


def test_conv_route_query_for_groupnorm_sums_is_host_only():
    """es_conv_emits_gn_stats: the planner's question "would this conv launch form the next GroupNorm's row-group sums in its own
    epilogue?" is answered on the host from the dispatcher's own routing (no launch, no device): yes for the 256-row
    producer/consumer tiles of a 32-object scene, no for few objects (split K / small tiles), for the GEGLU projection, for volumes
    with fewer than 64 voxels per object; a deterministic shard (O_hint) is asked about the WHOLE problem by the planner."""
    import ctypes as C
    from echoscene_amd import hip
    L = hip.lib()

    def args(O, dims, Cin, N, taps=27, epilogue=0, f32=True):
        a = hip.ConvArgs()
        a.a, a.w = 0x1000, 0x2000                      # never dereferenced by the query
        a.O, a.D, a.H, a.W = O, dims[0], dims[1], dims[2]
        a.Cin, a.N, a.taps, a.mode = Cin, N, taps, 0
        a.out_f32 = 0x3000 if f32 else None
        a.out_f16 = None if f32 else 0x4000
        a.bias = 0x5000
        a.out_ld = N if not epilogue else N // 2
        a.workspace, a.splitk = 0x6000, -1
        a.epilogue = epilogue
        return a
    assert L.es_conv_emits_gn_stats(C.byref(args(32, (16, 16, 16), 224, 224))) == 1
    assert L.es_conv_emits_gn_stats(C.byref(args(32, (16, 8, 8), 448, 448))) == 1
    assert L.es_conv_emits_gn_stats(C.byref(args(4, (16, 16, 16), 224, 224))) == 0        # 64 tiles: K split over workgroups
    assert L.es_conv_emits_gn_stats(C.byref(args(32, (16, 4, 4), 672, 672))) == 0         # 96 tiles at the 16x4x4 level
    assert L.es_conv_emits_gn_stats(C.byref(args(32, (16, 8, 8), 448, 3584, taps=1, epilogue=hip.EPI_GEGLU, f32=False))) == 0
    assert L.es_conv_emits_gn_stats(C.byref(args(4096, (2, 4, 4), 64, 224))) == 0         # 32 voxels per object
    bad = args(32, (16, 16, 16), 100, 224)                                                # Cin not a multiple of 32
    assert L.es_conv_emits_gn_stats(C.byref(bad)) == -1 and b'Cin' in L.es_last_error()
    # the other way a producer helps the next GroupNorm: a launch split over K forms that GroupNorm's per-tile partial sums in its
    # reduction kernel (gn_part_out) -- exactly the launches above that are too small for the epilogue sums
    def part(O, dims, cin, n, **kw):
        a = args(O, dims, cin, n, **kw)
        a.gn_part_groups = 32
        return a
    assert L.es_conv_emits_gn_part(C.byref(part(32, (16, 16, 16), 224, 224))) == 0
    assert L.es_conv_emits_gn_part(C.byref(part(4, (16, 16, 16), 224, 224))) == 1
    assert L.es_conv_emits_gn_part(C.byref(part(32, (16, 4, 4), 672, 672))) == 1
    assert L.es_conv_emits_gn_part(C.byref(args(4, (16, 16, 16), 224, 224))) == 0           # no group count given
    assert L.es_conv_emits_gn_part(C.byref(bad)) == -1


def test_conv_split_of_reports_the_slabs_a_launch_writes():
    """es_conv_split_of (round 6): how many fp32 slabs a launch writes into `workspace` -- the planner sizes the workspace with it.  A
    32-object launch of the 16^3 / 16x8x8 levels writes none; 4 objects split 2 / 4 / 8 ways on 128-row tiles; O_hint = -4 (the
    canonical arithmetic) gives every object count the reference shard's splits; a K-short linear on k_conv_kw writes none (its four
    K streams meet in LDS); a launch too large for 31-bit offsets is chunked and reports its chunks' slabs in units of its own M x N."""
    import ctypes as C
    from echoscene_amd import hip
    L = hip.lib()

    def args(O, dims, Cin, N, taps=27, oh=0):
        a = hip.ConvArgs()
        a.a, a.w = 0x1000, 0x2000
        a.O, a.D, a.H, a.W = O, dims[0], dims[1], dims[2]
        a.Cin, a.N, a.taps, a.mode = Cin, N, taps, 0
        a.out_f32, a.bias, a.out_ld = 0x3000, 0x5000, N
        a.workspace, a.splitk, a.O_hint = 0x6000, -1, oh
        return a
    lv = [((16, 16, 16), 672, 224), ((16, 8, 8), 448, 448), ((16, 4, 4), 672, 672)]
    f = lambda O, oh: [L.es_conv_split_of(C.byref(args(O, d, ci, n, oh=oh))) for d, ci, n in lv]
    assert f(32, 0) == [1, 1, 2] and f(4, 0) == [2, 4, 8]
    assert f(32, -4) == f(4, 0) == f(4, -4) == f(256, -4)
    assert L.es_conv_split_of(C.byref(args(4, (16, 8, 8), 448, 448, taps=1))) == 1          # k_conv_kw: no slabs
    big = args(1024, (16, 16, 16), 672, 224, oh=-4)                                           # 5.6 GB of input: chunks of 390 objects
    assert L.es_conv_split_of(C.byref(big)) == 1                                              # ceil(2 slabs x 390 / 1024)
    bad = args(4, (16, 16, 16), 100, 224)
    assert L.es_conv_split_of(C.byref(bad)) == -1


def test_route_options_are_explicit_and_recorded(L, tmp_path):
    """VERDICT r4 #6 / ADVICE r4: everything that decides where an fp32 sum is cut is a process-wide OPTION with a constant default,
    set only through the API -- the library reads no environment variable for it -- and the options string is what es_model_save writes
    behind the header of a model file (es_model_load compares it with the loading process's)."""
    import ctypes as C
    import os
    import re
    buf = C.create_string_buffer(1024)
    assert L.es_options_string(buf, 1024) > 0
    s = buf.value.decode()
    opts = dict(kv.split('=') for kv in s.strip(';').split(';'))
    assert opts == {'rows_family': '1', 'conv_tile': '0', 'conv_force256': '0', 'conv_ws': '1', 'conv_wssplit': '1', 'conv_wss_target': '256',
                    'conv_deep': '1', 'conv_tinysplit': '1', 'gn_rg': '1',
                    # round 6: the few-objects routes (1 = on) and the tools-only forcing switches (0 / defaults = off)
                    'conv_few': '1', 'conv_st_bm': '0', 'conv_st_np': '4', 'conv_st_ns': '3', 'conv_kw_ks': '0'}, opts
    # set / read back / restore; unknown names are errors
    assert L.es_vol_set_option(b'conv_wss_target', 512) == 0
    L.es_options_string(buf, 1024)
    assert 'conv_wss_target=512;' in buf.value.decode()
    assert L.es_vol_set_option(b'conv_wss_target', 256) == 0
    assert L.es_vol_set_option(b'no_such_option', 1) != 0
    # the environment is not consulted: the old switch names change nothing
    for name in ('ES_CONV_WSSPLIT', 'ES_CONV_TINYSPLIT', 'ES_CONV_WSS_TARGET', 'ES_CONV_DEEP', 'ES_GN_RG', 'ES_CONV_WS', 'ES_CONV_TILE', 'ES_CONV_FORCE256'):
        os.environ[name] = '0'
    try:
        L.es_options_string(buf, 1024)
        assert buf.value.decode() == s
    finally:
        for name in ('ES_CONV_WSSPLIT', 'ES_CONV_TINYSPLIT', 'ES_CONV_WSS_TARGET', 'ES_CONV_DEEP', 'ES_GN_RG', 'ES_CONV_WS', 'ES_CONV_TILE', 'ES_CONV_FORCE256'):
            del os.environ[name]
    # no getenv of a numerics-affecting switch is left in the sources: the remaining ones are listed as timing-only / debugging
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    allowed = {'ES_CONV_N16', 'ES_CONV_LINWS', 'ES_LIN_RING', 'ES_LIN_NCB_MAX', 'ES_CONV_NS', 'ES_CONV_A3', 'ES_CONV_GB', 'ES_DEBUG_SYNC', 'ES_ROWS_FUSE', 'ES_ROWS_PREFETCH', 'ES_ROWS_NT2', 'ES_ROWS_U1', 'ES_ROWS_DBG'}
    found = set()
    for f in os.listdir(os.path.join(here, 'echoscene_amd', 'csrc')):
        if f.endswith(('.hip', '.h')):
            found |= set(re.findall(r'getenv\("(\w+)"\)', open(os.path.join(here, 'echoscene_amd', 'csrc', f)).read()))
    assert found <= allowed, found - allowed
    # a model file carries the string right behind its 32-byte header (format 'ESMODEL2'): es_model_file_options reads it back
    path = str(tmp_path / 'fake.esmodel')
    with open(path, 'wb') as fp:
        fp.write(b'ESMODEL2' + bytes(24) + s.encode().ljust(512, b'\0'))
    out = C.create_string_buffer(1024)
    assert L.es_model_file_options(path.encode(), out, 1024) == 0 and out.value.decode() == s
