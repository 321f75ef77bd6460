"""CPU-only checks of box-preserving sampling (the masked ancestral layout loop): the additions to the C ABI, the schedule's two
q_sample columns, the keep plan next to the unmasked one, the unmasked op list against a record made on the commit before this
feature, and the argument errors of the public calls.  No device compute is called here (the library builds and loads on a CPU box,
as test_abi.py relies on)."""
import ctypes as C
import inspect
import json
import os
import subprocess

import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


def test_keep_struct_size_and_op_kind_match_header(L, tmp_path):
    """sizeof(es_ddpm_keep_args) as the C compiler sees it == the ctypes mirror; the new member is not the union's largest, so es_op
    (and with it the model-file format) keeps its size; es_update_args is untouched; ABI still 10.  The op kind is 21: kind 20 is left
    unassigned because tests/test_keep_cpu.py pins es_op_pointer_offsets(20) to "unknown kind"."""
    from echoscene_amd import hip
    names = {'es_ddpm_keep_args': hip.DdpmKeepArgs, 'es_op': hip.Op, 'es_update_args': hip.UpdateArgs, 'es_linear_args': hip.LinearArgs}
    src = '#include <stdio.h>\n#include "echoscene_hip.h"\nint main(){' + ''.join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + 'printf("keep %d\\n", ES_OP_DDPM_KEEP);return 0;}'
    c = tmp_path / 'sz.c'
    c.write_text(src)
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    vals = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert vals[n] == C.sizeof(cls), '%s: C %d vs ctypes %d' % (n, vals[n], C.sizeof(cls))
    assert vals['keep'] == hip.OP_DDPM_KEEP == 21
    assert C.sizeof(hip.UpdateArgs) == 80
    assert C.sizeof(hip.DdpmKeepArgs) < C.sizeof(hip.LinearArgs) <= C.sizeof(hip.Op) - 8
    assert C.sizeof(hip.Op) == 488, 'es_op grew: model files of the parent commit would no longer load'
    # the fields of es_update_args come first, at the same offsets: the generated rows' half of the kernel reads the same layout
    for name, _ in hip.UpdateArgs._fields_:
        assert getattr(hip.DdpmKeepArgs, name).offset == getattr(hip.UpdateArgs, name).offset, name
    assert L.es_abi_version() == 10


def test_keep_op_has_a_pointer_table_of_nine(L):
    """model files relocate the device pointers of the new op through es_op_pointer_offsets: exactly its nine c_void_p fields"""
    from echoscene_amd import hip
    u_off = hip.Op.u.offset
    buf = (C.c_size_t * 64)()
    n = L.es_op_pointer_offsets(hip.OP_DDPM_KEEP, buf, 64)
    want = sorted(u_off + getattr(hip.DdpmKeepArgs, name).offset for name, typ in hip.DdpmKeepArgs._fields_ if typ is C.c_void_p)
    assert n == 9 == len(want) and sorted(buf[i] for i in range(n)) == want
    assert {name for name, typ in hip.DdpmKeepArgs._fields_ if typ is C.c_void_p} == \
        {'x', 'eps', 'noise', 'coef', 'step', 'x0', 'mask', 'keep_noise', 'tab'}
    assert L.es_op_pointer_offsets(22, buf, 64) == -1


def test_new_symbols_are_declared_and_exported(L):
    from echoscene_amd import hip
    hdr = open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read()
    raw = C.CDLL(hip.LIB_PATH)
    for name in ('es_ddpm_update_keep', 'es_box_prescale', 'es_layout_sample_keep'):
        assert name + '(' in hdr and name in hip.EXPORTS and hasattr(raw, name), name
    assert 'ES_OP_DDPM_KEEP = 21' in hdr and 'typedef struct es_ddpm_keep_args' in hdr


def test_launchers_refuse_bad_arguments_on_the_host(L):
    """argument checks run before anything is enqueued: a bad call returns non-zero with a message (no device needed)"""
    from echoscene_amd import hip
    a = hip.DdpmKeepArgs()
    assert L.es_ddpm_update_keep(C.byref(a), None) != 0 and b'es_ddpm_update_keep' in L.es_last_error()
    for f in ('x', 'eps', 'noise', 'coef', 'step', 'x0', 'mask', 'keep_noise', 'tab'):
        setattr(a, f, 4096)
    a.n, a.row, a.n_tab, a.coef_stride, a.noise_stride, a.keep_noise_stride = 20, 8, 100, 5, 24, 24      # n no multiple of row
    assert L.es_ddpm_update_keep(C.byref(a), None) != 0
    a.n, a.keep_noise_stride = 24, 16                                                                    # a draw shorter than the state
    assert L.es_ddpm_update_keep(C.byref(a), None) != 0
    a.keep_noise_stride, a.n_tab = 24, 0                                                                 # an empty schedule
    assert L.es_ddpm_update_keep(C.byref(a), None) != 0
    assert L.es_box_prescale(None, 0, 6, None, None, None, 0, None, 4, None) != 0 and b'es_box_prescale' in L.es_last_error()
    assert L.es_box_prescale(4096, 7, 5, None, 4096, 4096, 7, None, 4, None) != 0                        # 5 columns: not a box
    assert L.es_layout_sample_keep(None, None, 0, 0, None, None, None, None, None) != 0


@pytest.mark.parametrize('T', [100, 1000])
def test_layout_schedule_q_sample_columns_equal_the_reference_tables(T):
    """LayoutSchedule.keep_tab = the reference GaussianDiffusion's sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod
    (diffusion_ddpm.py:147-148), bit for bit, in iteration order (iteration i <-> t = T-1-i); ``coef`` is what it was."""
    from echoscene_amd.schedules import LayoutSchedule
    g = load_golden('layout_keep_tiny')
    s = LayoutSchedule(T)
    assert tuple(s.keep_tab.shape) == (T, 2) and s.keep_tab.dtype == torch.float32 and tuple(s.coef.shape) == (T, 5)
    order = torch.arange(T - 1, -1, -1)
    assert torch.equal(s.keep_tab[:, 0], g['sac%d' % T][order])
    assert torch.equal(s.keep_tab[:, 1], g['s1mac%d' % T][order])
    if T == 100:
        ref = load_golden('layout_loop_tiny')
        assert torch.equal(s.coef[:, 0], ref['tab100_sqrt_recip_alphas_cumprod'][order])


# ------------------------------------------------------------------------------------------------ plans, without a device
def dry_layout_ops(keep=False, clip=False, O=8, T=100, mc=128):
    """The op list LayoutDenoiser._plan_for builds -- samplers.emit_layout_step, the function it calls -- emitted by a CPU Builder
    (tools/plan_dryrun.py's way: no plan is created, nothing runs): one UNet1D step with per-schedule tables and the K-sliced output
    conv, then the update op."""
    from echoscene_amd import synth, config as escfg
    from echoscene_amd.model.unet import UNet1DModel
    from echoscene_amd.plan import Builder, GraphIndex, UNet1DWeights
    from echoscene_amd.samplers import _cap, _cpu_sd, emit_layout_step
    from echoscene_amd.schedules import LayoutSchedule
    dev = torch.device('cpu')
    net = UNet1DModel(**escfg.layout_denoiser_kwargs(mc))
    synth.seeded_fill_(net, prefix='dry.')
    w = UNet1DWeights(_cpu_sd(net), net, dev)
    _, triples = synth.synthetic_graph(O, seed=3)
    g = GraphIndex(triples, O, dev, capacity=_cap(triples.shape[0]))
    sched = LayoutSchedule(T)
    b = Builder(dev)
    tables = dict(emb=None, emb_all=torch.zeros(T, w.emb_all.N), t_lin=torch.zeros(T, 64))
    emit_layout_step(b, w, g, torch.zeros(O, 640), torch.zeros(T, mc), tables, T, sched.coef, sched.keep_tab, clip=clip, keep=keep)
    return b.ops


def layout_op_signature(ops):
    """op_signature of tests/test_hip_keep.py (what 'op for op the same plan' means) on a bare op list"""
    from test_hip_keep import op_signature

    class _P:
        _arr = ops
    return op_signature(_P)


@pytest.fixture(scope='module')
def dry(L):
    return {k: dry_layout_ops(keep=k) for k in (False, True)}


def test_unmasked_layout_plan_is_the_parent_commits(dry):
    """without a mask the layout step's op list is, op for op, that of the commit before this feature
    (tests/golden/layout_plan_ops_tiny.json: recorded there with this file's dry_layout_ops + op_signature)"""
    from echoscene_amd import hip
    with open(os.path.join(HERE, 'golden', 'layout_plan_ops_tiny.json')) as f:
        parent = json.load(f)
    sig = layout_op_signature(dry[False])
    assert sig == parent['ops'], 'the mask=None layout plan differs from the plan of the parent commit'
    assert all(s[0] != hip.OP_DDPM_KEEP for s in sig) and sig[-1][0] == hip.OP_DDPM
    from echoscene_amd.plan import count_launches
    assert count_launches(dry[False]) == parent['n_launches']


def test_keep_plan_is_the_unmasked_plan_with_the_last_op_replaced(dry):
    """... and it makes the same number of launches: the masked loop adds none to the latency-bound layout step"""
    from echoscene_amd import hip
    from echoscene_amd.plan import count_launches
    plain, keep = dry[False], dry[True]
    sp, sk = layout_op_signature(plain), layout_op_signature(keep)
    assert len(sp) == len(sk) and sk[:-1] == sp[:-1]
    assert sp[-1][0] == hip.OP_DDPM and sk[-1][0] == hip.OP_DDPM_KEEP
    up, uk = plain[-1].u.update, keep[-1].u.keep
    for name, _ in hip.UpdateArgs._fields_:
        if name not in ('x', 'eps', 'noise', 'coef', 'step'):           # (pointers: each builder allocated its own buffers)
            assert getattr(up, name) == getattr(uk, name), name
    assert (uk.n, uk.row, uk.n_tab, uk.keep_noise_stride, uk.inc_step) == (64, 8, 100, 64, 1)
    assert count_launches(keep) == count_launches(plain)
    # beyond 4096 state elements both updates are followed by the separate step increment: two launches each
    for n, extra in ((4096, 0), (4104, 1)):
        a, b = hip.Op(), hip.Op()
        a.kind, b.kind = hip.OP_DDPM, hip.OP_DDPM_KEEP
        a.u.update.n = b.u.keep.n = n
        a.u.update.inc_step = b.u.keep.inc_step = 1
        assert count_launches([a]) == count_launches([b]) == 1 + extra
    b.u.keep.inc_step = 0
    assert count_launches([b]) == 1


# ------------------------------------------------------------------------------------------------ the public interface
def test_sample_signatures_take_the_box_keywords():
    from echoscene_amd.model import scene
    from echoscene_amd.samplers import LayoutDenoiser, sample_layout_and_shape
    for fn in (scene.Sg2ScDiffModel.sample, scene.Sg2ScDiffModel.sample_with_changes, scene.Sg2ScDiffModel.sample_with_additions,
               scene.Sg2BoxDiffModel.sampleBoxes, scene.Sg2BoxDiffModel.sampleBoxes_with_changes,
               scene.Sg2BoxDiffModel.sampleBoxes_with_additions):
        ps = inspect.signature(fn).parameters
        for k in ('keep_box_nodes', 'keep_boxes', 'keep_box_noise'):
            assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None, (fn.__name__, k)
    ps = inspect.signature(LayoutDenoiser.sample).parameters
    assert all(ps[k].default is None for k in ('x0', 'mask', 'keep_noise'))
    ps = inspect.signature(sample_layout_and_shape).parameters
    assert all(ps[k].default is None for k in ('box_x0', 'box_mask', 'box_keep_noise'))
    ps = inspect.signature(LayoutDenoiser.save_model).parameters
    assert ps['keep'].default is False


def _scene_model(typ):
    from echoscene_amd import synth, config as escfg
    from model.SGDiff import SGDiff
    return SGDiff(typ, escfg.tiny_diff_opt('cpu'), synth.VOCAB, replace_latent=False, with_changes=True, residual=True,
                  gconv_pooling='avg', with_angles=True, clip=True, separated=False)


def test_box_keep_argument_errors():
    """one of keep_box_nodes / keep_boxes without the other, a wrong shape, a noise table without nodes: ValueError before any device
    work; duplicates and out-of-range entries follow keep_selection; the shape-keeping errors are what they were"""
    m = _scene_model('echolayout')
    d = m.diff
    dev = torch.device('cpu')
    boxes = torch.arange(16, dtype=torch.float32).reshape(2, 8) / 16
    with pytest.raises(ValueError):
        d._box_keep([1, 3], None, None, 6, dev)
    with pytest.raises(ValueError):
        d._box_keep(None, boxes, None, 6, dev)
    with pytest.raises(ValueError):
        d._box_keep([1, 3], boxes[:, :6], None, 6, dev)               # metric [K, 6] rows are not the normalised [K, 8] state
    with pytest.raises(ValueError):
        d._box_keep([1, 3, 4], boxes, None, 6, dev)                   # one row per entry
    with pytest.raises(ValueError):
        d._box_keep([1, 3], boxes.reshape(-1), None, 6, dev)
    with pytest.raises(ValueError):
        d._box_keep(None, None, torch.zeros(100, 6, 8), 6, dev)
    assert d._box_keep(None, None, None, 6, dev) == {}
    kw = d._box_keep([3, 1], boxes, None, 6, dev)
    assert kw['mask'].tolist() == [0, 1, 0, 1, 0, 0] and kw['keep_noise'] is None
    assert torch.equal(kw['x0'][3], boxes[0]) and torch.equal(kw['x0'][1], boxes[1]) and not kw['x0'][[0, 2, 4, 5]].any()
    kw2 = d._box_keep(torch.tensor([3, 1, 3, 17, -2]), torch.cat([boxes, boxes * 0 + 9, boxes[:1] * 0 + 9]), None, 6, dev)
    assert torch.equal(kw2['x0'], kw['x0']) and torch.equal(kw2['mask'], kw['mask'])
    # the errors in front of the device work of the facade: raised on a CPU model, before the HIP path is asked for
    a = (torch.zeros(6, dtype=torch.long), torch.zeros(5, 3, dtype=torch.long), torch.zeros(6, 512), torch.zeros(5, 512))
    with pytest.raises(ValueError, match='SHAPES'):
        m.sample_box_and_shape(*a, keep_nodes=[1], keep_sdfs=torch.zeros(1, 1, 64, 64, 64))     # _no_keep_without_shapes still fires
