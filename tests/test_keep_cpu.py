"""CPU-only checks of shape-preserving sampling (VQ-VAE encoder + masked DDIM): the additions to the C ABI, the host-only route
query of the new conv mode, the schedule's two q_sample columns, the fp64 fold of quant_conv and the keep_nodes -> mask rule.
No device compute is called here (the library builds and loads on a CPU box, as test_abi.py relies on)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


def test_new_struct_sizes_match_header(L, tmp_path):
    """sizeof() of the new argument structs as the C compiler sees them == the ctypes mirrors; es_op did not grow; ABI still 10."""
    from echoscene_amd import hip
    names = {'es_blend_args': hip.BlendArgs, 'es_conv_c1_args': hip.ConvC1Args, 'es_op': hip.Op, 'es_update_args': hip.UpdateArgs}
    src = '#include <stdio.h>\n#include "echoscene_hip.h"\nint main(){' + ''.join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + \
        'printf("mode %d\\n", ES_CONV_DOWN_DHW_P01); printf("blend %d\\n", ES_OP_DDIM_BLEND); printf("c1 %d\\n", ES_OP_CONV_C1);return 0;}'
    c = tmp_path / 'sz.c'
    c.write_text(src)
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    vals = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert vals[n] == C.sizeof(cls), '%s: C %d vs ctypes %d' % (n, vals[n], C.sizeof(cls))
    # es_update_args is what it was (80 bytes) and the new union members are not the largest: es_op keeps its size
    assert C.sizeof(hip.UpdateArgs) == 80
    assert max(C.sizeof(hip.BlendArgs), C.sizeof(hip.ConvC1Args)) < C.sizeof(hip.LinearArgs) <= C.sizeof(hip.Op) - 8
    assert (vals['mode'], vals['blend'], vals['c1']) == (hip.CONV_DOWN_DHW_P01, hip.OP_DDIM_BLEND, hip.OP_CONV_C1) == (5, 18, 19)
    assert L.es_abi_version() == 10


def test_new_op_kinds_have_pointer_tables(L):
    """model files relocate the device pointers of the new ops through es_op_pointer_offsets: exactly the c_void_p fields"""
    from echoscene_amd import hip
    u_off = hip.Op.u.offset
    buf = (C.c_size_t * 64)()
    for kind, struct in ((hip.OP_DDIM_BLEND, hip.BlendArgs), (hip.OP_CONV_C1, hip.ConvC1Args)):
        n = L.es_op_pointer_offsets(kind, buf, 64)
        want = sorted(u_off + getattr(struct, name).offset for name, typ in struct._fields_ if typ is C.c_void_p)
        assert n == len(want) and sorted(buf[i] for i in range(n)) == want, struct.__name__
    assert L.es_op_pointer_offsets(99, buf, 64) == -1 and L.es_op_pointer_offsets(20, buf, 64) == -1


def _conv_query(mode, O=1, dims=(16, 16, 16), Cin=128, N=128):
    from echoscene_amd import hip
    a = hip.ConvArgs()
    a.a, a.w, a.out_f32 = 4096, 4096, 4096           # (host-only query: only asked whether they are there)
    a.O, (a.D, a.H, a.W) = O, dims
    a.Cin, a.N, a.taps, a.mode = Cin, N, 27, mode
    a.out_ld, a.splitk, a.workspace = N, -1, 4096
    return a


def test_conv_mode_5_is_routed_and_unknown_modes_are_refused(L):
    from echoscene_amd import hip
    for O, dims, Cin in ((1, (16, 16, 16), 128), (8, (32, 32, 32), 64), (2, (16, 16, 16), 64)):
        a = _conv_query(hip.CONV_DOWN_DHW_P01, O, dims, Cin, Cin)
        b = _conv_query(hip.CONV_DOWN_DHW, O, dims, Cin, Cin)
        s5, s4 = L.es_conv_split_of(C.byref(a)), L.es_conv_split_of(C.byref(b))
        assert s5 >= 1, L.es_last_error()
        assert s5 == s4                              # same geometry, same K: the route does not depend on where the padding sits
    for bad in (6, 7, -1, 99):
        a = _conv_query(bad)
        assert L.es_conv_split_of(C.byref(a)) == -1
        assert b'mode' in L.es_last_error()


def test_launchers_refuse_bad_arguments_on_the_host(L):
    """argument checks run before anything is enqueued: a bad call returns non-zero with a message (no device needed)"""
    from echoscene_amd import hip
    a = hip.BlendArgs()
    assert L.es_ddim_blend(C.byref(a), None) != 0 and b'es_ddim_blend' in L.es_last_error()
    a.x = a.x0 = a.mask = a.noise = a.tab = a.step = 4096
    a.O, a.n, a.noise_stride = 4, 12286, 4 * 12288          # n % 4 != 0
    assert L.es_ddim_blend(C.byref(a), None) != 0
    a.n, a.noise_stride = 12288, 12288                       # the stride does not cover O objects
    assert L.es_ddim_blend(C.byref(a), None) != 0
    c = hip.ConvC1Args()
    c.x = c.w = c.out_f32 = 4096
    c.O, c.D, c.H, c.W, c.N = 1, 64, 64, 64, 48              # 48 channels: no kernel
    assert L.es_conv_c1_f32(C.byref(c), None) != 0 and b'N=48' in L.es_last_error()
    c.N, c.W = 64, 40                                        # W not a multiple of 16
    assert L.es_conv_c1_f32(C.byref(c), None) != 0


@pytest.mark.parametrize('S', [4, 100])
def test_schedule_q_sample_columns_equal_the_models_tables(S):
    """ShapeSchedule.keep_tab = the reference model's sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod at the DDIM timesteps, bit
    for bit, in iteration order; ``coef`` and its stride are what they were."""
    from echoscene_amd.schedules import ShapeSchedule
    g = load_golden('ddim_keep_tiny')
    s = ShapeSchedule(S)
    assert tuple(s.keep_tab.shape) == (S, 2) and s.keep_tab.dtype == torch.float32 and tuple(s.coef.shape) == (S, 4)
    assert np.array_equal(s.ddim_timesteps, g['ts%d' % S].numpy())
    order = torch.arange(S - 1, -1, -1)
    assert torch.equal(s.keep_tab[:, 0], g['sac%d' % S][order])
    assert torch.equal(s.keep_tab[:, 1], g['s1mac%d' % S][order])
    assert tuple(ShapeSchedule(S, eta=0.7).coef.shape) == (S, 5)


def test_quant_conv_folds_into_conv_out_in_fp64():
    from echoscene_amd import config as escfg, synth
    from echoscene_amd.model.vqvae import VQVAE
    from echoscene_amd.plan_vol import fold_quant_conv
    p = escfg.vqvae_conf(32).model.params
    vq = VQVAE(dict(p.ddconfig), 64, p.embed_dim)
    synth.seeded_fill_(vq, prefix='vqvae_tiny.')
    sd = {k: v.detach() for k, v in vq.state_dict().items()}
    Wf, bf = fold_quant_conv(sd)
    assert Wf.dtype == torch.float64 and tuple(Wf.shape) == (p.embed_dim, sd['encoder.conv_out.weight'].shape[1], 3, 3, 3)
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((2, Wf.shape[1], 5, 6, 7)))
    ref = F.conv3d(F.conv3d(x, sd['encoder.conv_out.weight'].double(), sd['encoder.conv_out.bias'].double(), padding=1),
                   sd['quant_conv.weight'].double(), sd['quant_conv.bias'].double())
    got = F.conv3d(x, Wf, bf, padding=1)
    err = (got - ref).abs().max().item()
    print('fold of quant_conv into conv_out: max abs err %.3e (|ref| max %.3f)' % (err, ref.abs().max()))
    assert err < 1e-12
    sd2 = dict(sd)
    sd2['encoder.conv_out.weight'] = torch.cat([sd['encoder.conv_out.weight']] * 2, 0)       # double_z: twice the channels
    with pytest.raises(NotImplementedError):
        fold_quant_conv(sd2)


def test_keep_nodes_to_mask():
    """duplicates and out-of-range entries follow the manipulated_nodes convention: a node counts once (its first entry names its
    SDF), entries outside [0, O) are ignored"""
    from echoscene_amd.samplers import keep_selection
    mask, rows, src = keep_selection([3, 1], 6)
    assert mask.tolist() == [0, 1, 0, 1, 0, 0] and rows == [1, 3] and src == [1, 0]
    mask2, rows2, src2 = keep_selection([1, 3, 3, 17, -2], 6)
    assert torch.equal(mask2, mask) and rows2 == [1, 3] and src2 == [0, 1]
    mask3, rows3, src3 = keep_selection(torch.tensor([5, 5, 0]), 6)
    assert mask3.tolist() == [1, 0, 0, 0, 0, 1] and rows3 == [0, 5] and src3 == [2, 0]
    m0, r0, s0 = keep_selection([], 4)
    assert m0.tolist() == [0, 0, 0, 0] and r0 == [] and s0 == []


def test_sample_signatures_take_the_keywords():
    import inspect
    from echoscene_amd.model import scene
    from echoscene_amd.samplers import ShapeDenoiser, VQEncoder
    for fn in (scene.Sg2ScDiffModel.sample, scene.Sg2ScDiffModel.sample_with_changes, scene.Sg2ScDiffModel.sample_with_additions):
        ps = inspect.signature(fn).parameters
        for k in ('keep_nodes', 'keep_sdfs'):
            assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None
    ps = inspect.signature(ShapeDenoiser.sample).parameters
    assert all(ps[k].default is None for k in ('x0', 'mask', 'keep_noise'))
    assert 'encode_no_quant' in dir(VQEncoder)
