"""CPU-only checks of shape completion (per-voxel keep masks in the masked shape loop): the reference's range rule on the host, the
additions to the C ABI, the step the planner emits for the voxel form of the loop, and every refusal of the public keywords.
No device compute is called here (the library builds and loads on a CPU box, as test_abi.py relies on)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the six ranges of tests/golden/make_golden_complete.py with the bounds of the reference's rule at n = 16 and n = 64
TABLE = [
    (dict(x=(-1, 1), y=(-1, 0), z=(-1, 1)), [0, 16, 0, 8, 0, 16], [0, 64, 0, 32, 0, 64]),
    (dict(x=(-0.3, 0.45), y=(-1, 1), z=(-0.6, 1)), [5, 11, 0, 16, 3, 16], [22, 46, 0, 64, 12, 64]),
    (dict(x=(-2, 0.1), y=(-0.55, 3), z=(-0.9, 0.3)), [0, 8, 3, 16, 0, 10], [0, 35, 14, 64, 3, 41]),
    (dict(x=(0.5, -0.5), y=(-1, 1), z=(-1, 1)), [12, 4, 0, 16, 0, 16], [48, 16, 0, 64, 0, 64]),
    (dict(x=(-1, 1), y=(-1, 1), z=(-1, 1)), [0, 16] * 3, [0, 64] * 3),
    (dict(x=(0.2, 0.3), y=(0.2, 0.3), z=(0.2, 0.3)), [9, 10] * 3, [38, 41] * 3),
]


def golden_ranges(g):
    return [dict(x=(float(r[0]), float(r[1])), y=(float(r[2]), float(r[3])), z=(float(r[4]), float(r[5]))) for r in g['ranges'].numpy()]


def host_mask(bounds, n):
    """the 0/1 box [K, n, n, n] of integer bounds [K, 6]: st <= index < ed on all three axes"""
    i = np.arange(n)
    out = []
    for b in np.asarray(bounds):
        ax = [(i >= b[2 * a]) & (i < b[2 * a + 1]) for a in range(3)]
        out.append(ax[0][:, None, None] & ax[1][None, :, None] & ax[2][None, None, :])
    return np.stack(out)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


# ------------------------------------------------------------------------------------------------ the range rule
def test_range_bounds_reproduce_the_reference():
    """postprocess.range_bounds against the table of the six ranges and against the masks get_partial_shape itself produced
    (partial_shape_ranges): the bounds read back from the reference's masks where a mask is not empty, and the masks themselves --
    the empty range too -- at 16^3 and 64^3"""
    from echoscene_amd.postprocess import range_bounds
    g = load_golden('partial_shape_ranges')
    ranges = golden_ranges(g)
    assert len(ranges) == len(TABLE) == 6
    for (r, b16, b64), rg in zip(TABLE, ranges):
        assert {k: tuple(float(v) for v in r[k]) for k in r} == rg
    b16, b64 = range_bounds(ranges, 16), range_bounds(ranges, 64)
    assert b16.dtype == np.int32 and b16.shape == (6, 6)
    assert b16.tolist() == [t[1] for t in TABLE] and b64.tolist() == [t[2] for t in TABLE]
    assert range_bounds([t[0] for t in TABLE], 16).tolist() == b16.tolist()          # (int ends as the caller may write them)
    for k in range(6):
        for got, ref in ((b16[k], g['bounds16'][k].numpy()), (b64[k], g['bounds64'][k].numpy())):
            if ref[0] >= 0:
                assert got.tolist() == ref.tolist(), k
            else:
                assert any(got[2 * a] >= got[2 * a + 1] for a in range(3)), k
    assert np.array_equal(host_mask(b16, 16), g['z_mask'].numpy() != 0)
    bits = np.stack([np.packbits(m.reshape(-1)) for m in host_mask(b64, 64)])
    assert np.array_equal(bits, g['shape_mask_bits'].numpy())
    assert int(host_mask(b16, 16)[3].sum()) == 0 and int(host_mask(b16, 16)[5].sum()) == 1 and host_mask(b16, 16)[4].all()
    assert range_bounds(ranges[1], 16).tolist() == [TABLE[1][1]]                     # one dict: K = 1
    for bad in ([dict(x=(0, 1), y=(0, 1))], [((0, 1),) * 3], [dict(x=(0, 1), y=(0, 1), z=(0, 1), w=(0, 1))]):
        with pytest.raises(ValueError, match='range_bounds'):
            range_bounds(bad, 16)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_blend_vox_struct_op_kind_and_abi(L, tmp_path):
    """sizeof(es_blend_vox_args) as the C compiler sees it == the ctypes mirror; ES_OP_DDIM_BLEND_VOX == 28; es_op did not grow (488);
    ABI still 10"""
    from echoscene_amd import hip
    names = {'es_blend_vox_args': hip.BlendVoxArgs, 'es_blend_args': hip.BlendArgs, 'es_op': hip.Op}
    src = '#include <stdio.h>\n#include "echoscene_hip.h"\nint main(){' + ''.join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + \
        'printf("vox %d\\n", ES_OP_DDIM_BLEND_VOX); printf("abi %d\\n", ES_ABI_VERSION);return 0;}'
    c = tmp_path / 'sz.c'
    c.write_text(src)
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    vals = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert vals[n] == C.sizeof(cls), '%s: C %d vs ctypes %d' % (n, vals[n], C.sizeof(cls))
    assert vals['vox'] == hip.OP_DDIM_BLEND_VOX == 28
    assert vals['es_op'] == C.sizeof(hip.Op) == 488
    assert vals['abi'] == L.es_abi_version() == 10
    assert [n for n, _ in hip.BlendVoxArgs._fields_] == ['x', 'x0', 'mask', 'noise', 'noise_stride', 'tab', 'step', 'O', 'C', 'V']


def test_blend_vox_pointer_table_and_exports(L):
    """es_op_pointer_offsets(28) lists exactly the struct's pointer fields (model files relocate them); every function the header
    declares is in hip.EXPORTS, the three new ones among them"""
    from echoscene_amd import hip
    buf = (C.c_size_t * 64)()
    n = L.es_op_pointer_offsets(hip.OP_DDIM_BLEND_VOX, buf, 64)
    want = sorted(hip.Op.u.offset + getattr(hip.BlendVoxArgs, name).offset for name, typ in hip.BlendVoxArgs._fields_ if typ is C.c_void_p)
    assert n == len(want) == 6 and sorted(buf[i] for i in range(n)) == want
    assert all(L.es_op_pointer_offsets(k, buf, 64) == -1 for k in (20, 22, 26, 29))
    hdr = open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(es_[a-z0-9_]+)\s*\(', hdr))
    assert {'es_ddim_blend_vox', 'es_range_mask', 'es_partial_shape'} <= declared
    missing = sorted(declared - set(hip.EXPORTS))
    assert not missing, 'declared in the header, not bound in hip.EXPORTS: %s' % missing
    for name in ('es_ddim_blend_vox', 'es_range_mask', 'es_partial_shape'):
        assert getattr(L, name) is not None


def test_launchers_refuse_bad_arguments_on_the_host(L):
    """every pointer, the sizes, the stride, the alignment and the object count are checked before anything is enqueued"""
    from echoscene_amd import hip

    def good():
        a = hip.BlendVoxArgs()
        a.x = a.x0 = a.mask = a.noise = a.tab = a.step = 4096
        a.O, a.C, a.V, a.noise_stride = 4, 3, 4096, 4 * 3 * 4096
        return a
    fn = L.es_ddim_blend_vox
    assert fn(C.byref(hip.BlendVoxArgs()), None) != 0 and b'es_ddim_blend_vox' in L.es_last_error()
    assert fn(None, None) != 0
    for field in ('x', 'x0', 'mask', 'noise', 'tab', 'step'):
        a = good()
        setattr(a, field, None)
        assert fn(C.byref(a), None) != 0 and b'NULL' in L.es_last_error(), field
    for field, v in (('V', 4094), ('V', 0), ('C', 0), ('O', 0), ('noise_stride', 4 * 3 * 4096 - 4), ('noise_stride', 4 * 3 * 4096 + 2),
                     ('O', 65536)):
        a = good()
        if field == 'O' and v > 4:
            a.noise_stride = v * 3 * 4096
        setattr(a, field, v)
        assert fn(C.byref(a), None) != 0 and b'es_ddim_blend_vox' in L.es_last_error(), (field, v)
    for field in ('x', 'x0', 'mask', 'noise'):
        a = good()
        setattr(a, field, 4096 + 8)
        assert fn(C.byref(a), None) != 0 and b'aligned' in L.es_last_error(), field
    assert L.es_range_mask(None, 1, 16, 16, 16, 4096, None) != 0 and b'es_range_mask' in L.es_last_error()
    assert L.es_range_mask(4096, 0, 16, 16, 16, 4096, None) != 0
    assert L.es_range_mask(4096, 1, 16, 0, 16, 4096, None) != 0
    assert L.es_partial_shape(4096, 4096, 1, 64, C.c_float(0.2), 4096, 4096, None, None) != 0 and b'es_partial_shape' in L.es_last_error()
    assert L.es_partial_shape(4096, 4096, 1, 0, C.c_float(0.2), 4096, 4096, 4096, None) != 0


# ------------------------------------------------------------------------------------------------ the planner
_W = {}


def dry_shape_ops(**kw):
    """samplers.emit_shape_step -- the function ShapeDenoiser._build_state calls -- on a CPU Builder, for the tiny denoiser of the GPU
    tests: (kinds of the ops of the steady step, the emitter's result)"""
    from echoscene_amd import synth, config as escfg
    from echoscene_amd.model.unet import DiffusionUNet
    from echoscene_amd.plan import Builder, GraphIndex
    from echoscene_amd.plan_vol import UNet3DWeights
    from echoscene_amd.samplers import _cap, _cpu_sd, emit_shape_step
    dev = torch.device('cpu')
    if 'w' not in _W:
        p = escfg.shape_unet_params(32)
        p['context_dim'] = 64
        df = DiffusionUNet(p)
        synth.seeded_fill_(df, prefix='unet3d_tiny.')
        _W['w'] = UNet3DWeights({k[len('diffusion_net.'):]: v for k, v in _cpu_sd(df).items()}, df.diffusion_net, dev, 'fp16')
    w = _W['w']
    O, S = 4, 4
    _, triples = synth.synthetic_graph(O, seed=6)
    g = GraphIndex(triples, O, dev, capacity=_cap(triples.shape[0]))
    b = Builder(dev, shard_block=O, force_exchange=False, up_fold=True)
    tables = dict(emb=None, emb_all=torch.zeros(S, w.emb_all.N), t_lin=torch.zeros(S, 64))
    out = emit_shape_step(b, w, g, torch.zeros(O, 64), torch.zeros(S, w.mc), tables, torch.zeros(S, 4), torch.zeros(S, 2), S,
                          (3, 16, 16, 16), 0, O, gather_rows=O, **kw)
    return b.ops, out


def _kinds(ops):
    return [int(op.kind) for op in ops]


@pytest.mark.parametrize('plms', [False, True])
def test_voxel_step_is_the_plain_step_with_one_op_28_in_front(plms):
    """emit_shape_step(keep_vox=True): the plain step with ONE es_ddim_blend_vox in front, reading a mask [O, V]; under PLMS the
    composed first_plan has it once (before the first evaluation only); the plain and the per-object plans contain no op 28"""
    from echoscene_amd import hip
    from echoscene_amd.samplers import compose_step_plans
    plain, po = dry_shape_ops(plms=plms)
    keep, ko = dry_shape_ops(plms=plms, keep=True)
    vox, vo = dry_shape_ops(plms=plms, keep_vox=True)
    kp, kk, kv = _kinds(plain), _kinds(keep), _kinds(vox)
    assert hip.OP_DDIM_BLEND_VOX == 28 and 28 not in kp and 28 not in kk
    assert kv == [28] + kp and kk == [hip.OP_DDIM_BLEND] + kp
    assert (po['n_blend'], ko['n_blend'], vo['n_blend']) == (0, 1, 1)
    assert tuple(vo['mask'].shape) == (4, 4096) and tuple(ko['mask'].shape) == (4,) and float(vo['mask'].abs().sum()) == 0.0
    assert tuple(vo['x0'].shape) == (4, 3, 16, 16, 16) and tuple(vo['knoise'].shape) == tuple(ko['knoise'].shape) == (4, 4 * 12288)
    a = vox[0].u.blend_vox
    assert (a.O, a.C, a.V, a.noise_stride) == (4, 3, 4096, 4 * 12288)
    assert (a.x, a.x0, a.mask, a.noise, a.step) == (vo['x'].data_ptr(), vo['x0'].data_ptr(), vo['mask'].data_ptr(),
                                                    vo['knoise'].data_ptr(), vo['step'].data_ptr())
    # ``keep_vox`` alone asks for the masked loop; with ``keep`` it is the same step
    both, _ = dry_shape_ops(plms=plms, keep=True, keep_vox=True)
    assert _kinds(both) == kv
    plans = compose_step_plans(vox, vo['n_blend'], vo['split'], vo['n_eps_ops'], *vo['first_ops'], plms=plms, sharded=True)
    assert _kinds(plans['plan']).count(28) == 1 and _kinds(plans['stem_plan'])[0] == 28 and 28 not in _kinds(plans['main_plan'])
    if plms:
        first = _kinds(plans['first_plan'])
        assert first.count(28) == 1 and first[0] == 28
        assert first.count(hip.OP_PLMS_FIRST_A) == 1 and first.count(hip.OP_PLMS_FIRST_B) == 1
        assert 28 not in _kinds(plans['stem2_plan']) and 28 not in _kinds(plans['main_a_plan']) + _kinds(plans['main_b_plan'])
    else:
        assert plans['first_plan'] is None


# ------------------------------------------------------------------------------------------------ the mask forms of the loop owner
def test_shape_mask_forms():
    """ShapeDenoiser's mask: [O] (per object), [O, 1, D, H, W] or [O, D, H, W] (per voxel); anything else -- a mask per channel too --
    is a ValueError that says so"""
    from echoscene_amd.samplers import _check_shape_mask
    O, zs = 4, (3, 16, 16, 16)
    x0 = torch.zeros((O,) + zs)
    _, m, vox = _check_shape_mask(x0, torch.tensor([0, 1, 0, 1]), O, zs)
    assert not vox and m.tolist() == [0, 1, 0, 1] and m.dtype == torch.float32
    vm = torch.zeros(O, 1, 16, 16, 16)
    vm[1], vm[2, :, 5:11, :, 3:] = 1, 1
    for form in (vm, vm[:, 0], vm.bool(), vm.to(torch.uint8)):
        _, m, vox = _check_shape_mask(x0, form, O, zs)
        assert vox and tuple(m.shape) == (O, 4096) and m.dtype == torch.float32 and torch.equal(m, vm.reshape(O, -1))
    for bad in (vm.expand(O, 3, 16, 16, 16), vm[:3], vm[:, :, :8], torch.zeros(O, 2), torch.zeros(O + 1)):
        with pytest.raises(ValueError, match='per object.*per latent voxel'):
            _check_shape_mask(x0, bad, O, zs)
    with pytest.raises(ValueError, match='per channel'):
        _check_shape_mask(x0, vm.expand(O, 3, 16, 16, 16), O, zs)
    with pytest.raises(ValueError):
        _check_shape_mask(x0, vm * 0.5, O, zs)
    with pytest.raises(ValueError):
        _check_shape_mask(x0[:3], vm, O, zs)


# ------------------------------------------------------------------------------------------------ the public interface
def test_signatures_take_the_completion_keywords():
    from echoscene_amd.model import scene
    from echoscene_amd.samplers import emit_shape_step
    from echoscene_amd import postprocess
    for fn in (scene.Sg2ScDiffModel.sample, scene.Sg2ScDiffModel.sample_with_changes, scene.Sg2ScDiffModel.sample_with_additions):
        ps = inspect.signature(fn).parameters
        for k in ('complete_nodes', 'complete_sdfs', 'complete_ranges', 'complete_masks'):
            assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None, (fn.__name__, k)
    assert inspect.signature(emit_shape_step).parameters['keep_vox'].default is False
    assert inspect.signature(postprocess.partial_shape).parameters['fill'].default == 0.2
    assert list(inspect.signature(postprocess.latent_range_mask).parameters)[:3] == ['ranges', 'zdims', 'device']
    import model.SGDiff as facade
    assert facade.SGDiff is scene.SGDiff


def _scene_model(typ):
    from echoscene_amd import synth, config as escfg
    from model.SGDiff import SGDiff
    return SGDiff(typ, escfg.tiny_diff_opt('cpu'), synth.VOCAB, replace_latent=False, with_changes=True, residual=True,
                  gconv_pooling='avg', with_angles=True, clip=True, separated=False)


def test_completion_keyword_refusals_without_a_device():
    """every refusal is a ValueError raised before any device work, on all three calls: gen_shape=False, a node in both lists, ranges
    and masks both given or neither, wrong shapes, an 'echolayout' model"""
    m = _scene_model('echoscene')
    a = (None, None, None, None)
    sdf = torch.zeros(2, 1, 64, 64, 64)
    ranges = [TABLE[1][0], TABLE[2][0]]
    masks = torch.ones(2, 1, 16, 16, 16)
    ok = dict(complete_nodes=[1, 4], complete_sdfs=sdf, complete_ranges=ranges)
    cases = [
        ('gen_shape', dict(ok, gen_shape=False)),
        ('gen_shape', dict(ok)),                                                                     # (the calls' default: False)
        ('keep_nodes and in complete_nodes', dict(ok, gen_shape=True, keep_nodes=[4], keep_sdfs=sdf[:1])),
        ('exactly one', dict(ok, gen_shape=True, complete_masks=masks)),
        ('exactly one', dict(gen_shape=True, complete_nodes=[1, 4], complete_sdfs=sdf)),
        ('go together', dict(gen_shape=True, complete_nodes=[1, 4], complete_ranges=ranges)),
        ('go together', dict(gen_shape=True, complete_sdfs=sdf, complete_ranges=ranges)),
        ('go together', dict(gen_shape=True, complete_masks=masks)),
        ('complete_sdfs must be', dict(ok, gen_shape=True, complete_sdfs=sdf[:1])),
        ('complete_sdfs must be', dict(ok, gen_shape=True, complete_sdfs=sdf[:, 0])),
        ('complete_sdfs must be', dict(ok, gen_shape=True, complete_sdfs=sdf.expand(2, 3, 64, 64, 64))),
        ('complete_ranges must hold', dict(ok, gen_shape=True, complete_ranges=ranges[:1])),
        ('range_bounds', dict(ok, gen_shape=True, complete_ranges=[ranges[0], dict(x=(0, 1))])),
        ('complete_masks must be', dict(gen_shape=True, complete_nodes=[1, 4], complete_sdfs=sdf, complete_masks=masks[:1])),
        ('complete_masks must be', dict(gen_shape=True, complete_nodes=[1, 4], complete_sdfs=sdf, complete_masks=masks.expand(2, 3, 16, 16, 16))),
        ('complete_masks must be', dict(gen_shape=True, complete_nodes=[1, 4], complete_sdfs=sdf, complete_masks=masks[:, 0])),
        ('complete_masks must be', dict(gen_shape=True, complete_nodes=[1, 4], complete_sdfs=sdf, complete_masks=torch.ones(2, 1, 8, 8, 8))),
        ('0 \\(generate\\) or 1', dict(gen_shape=True, complete_nodes=[1, 4], complete_sdfs=sdf, complete_masks=masks * 0.5)),
    ]
    for match, kw in cases:
        with pytest.raises(ValueError, match=match):
            m.sample_box_and_shape(*a, **kw)
        with pytest.raises(ValueError, match=match):
            m.sample_boxes_and_shape_with_changes(*a, *a, [1], **kw)
        with pytest.raises(ValueError, match=match):
            m.sample_boxes_and_shape_with_additions(*a, *a, [1], **kw)
    # the scene model itself refuses too (a caller below the facade)
    with pytest.raises(ValueError, match='exactly one'):
        m.diff.ShapeDiff.check_complete([1], sdf[:1], None, None)
    # accepted forms come back normalised; nothing without the keywords
    S = m.diff.ShapeDiff
    assert S.check_complete() is None
    nodes, sd, rg, mk = S.check_complete(torch.tensor([1, 4]), sdf, ranges, None, keep_nodes=[6])
    assert nodes == [1, 4] and rg == ranges and mk is None
    nodes, sd, rg, mk = S.check_complete([1, 4], sdf, None, masks)
    assert rg is None and torch.equal(mk, masks)
    ml = _scene_model('echolayout')
    for kw in (dict(ok), dict(complete_masks=masks), dict(complete_nodes=[1])):
        with pytest.raises(ValueError, match="'echolayout' model has no shape branch"):
            ml.sample_box_and_shape(*a, **kw)
        with pytest.raises(ValueError, match="'echolayout' model has no shape branch"):
            ml.sample_boxes_and_shape_with_changes(*a, *a, [1], **kw)
        with pytest.raises(ValueError, match="'echolayout' model has no shape branch"):
            ml.sample_boxes_and_shape_with_additions(*a, *a, [1], **kw)
