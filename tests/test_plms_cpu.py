"""CPU-only checks of PLMS shape sampling: the host-side evaluation sequence against what the reference's PLMSSampler recorded
(tests/golden/make_golden_plms.py), the additions to the C ABI, argument validation of the new keywords, and the extended shard
protocol on 2 and 3 gloo ranks with a toy backend that counts collectives.  No device compute is called here."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


# ------------------------------------------------------------------------------------------------ evaluation sequence, goldens
@pytest.mark.parametrize('S', [4, 5])
def test_evaluation_sequence_is_the_references(S):
    """schedules.plms_evaluations(S) -> the timesteps the reference's PLMSSampler called the denoiser at, in order: S + 1 calls, the
    second one at the NEXT timestep (t_next), which the first steady iteration then evaluates again."""
    from echoscene_amd.schedules import ShapeSchedule, plms_evaluations
    g = load_golden('plms_tiny')
    s = ShapeSchedule(S)
    ev = plms_evaluations(len(s.timesteps))
    assert len(ev) == S + 1
    assert [int(s.timesteps[row]) for row, _ in ev] == g['S%d_calls' % S].tolist()
    assert [k for _, k in ev] == ['first', 'second'] + ['steady'] * (S - 1)
    assert [row for row, _ in ev] == [0, 1] + list(range(1, S))
    assert np.array_equal(s.ddim_timesteps, g['S%d_ddim_timesteps' % S].numpy())
    # n_steps counts ITERATIONS: k iterations are k + 1 evaluations
    assert plms_evaluations(S, 0) == [] and plms_evaluations(S, 1) == ev[:2] and plms_evaluations(S, 3) == ev[:4]
    with pytest.raises(ValueError):
        plms_evaluations(1)
    with pytest.raises(ValueError):
        plms_evaluations(S, S + 1)


def test_issue_figures_of_the_recorded_calls():
    g = load_golden('plms_tiny')
    assert g['S4_calls'].tolist() == [751, 501, 501, 251, 1]
    assert g['S5_calls'].tolist() == [801, 601, 601, 401, 201, 1]


def test_golden_files_load_and_are_consistent():
    from echoscene_amd.schedules import ShapeSchedule
    g, gk, gs, gd = load_golden('plms_tiny'), load_golden('plms_keep_tiny'), load_golden('scene_plms_tiny'), load_golden('ddim_tiny')
    assert torch.equal(g['uc_s'], gd['uc_s']) and torch.equal(g['triples'], gd['triples'])       # the inputs of ddim_tiny
    for S in (4, 5):
        z, sub, ab = g['S%d_z_final' % S], g['S%d_states_sub' % S], g['S%d_states_abs' % S]
        assert tuple(z.shape) == (4, 3, 16, 16, 16) and tuple(sub.shape) == (S, 4, 3, 4, 4, 4) and tuple(ab.shape) == (S,)
        assert torch.equal(sub[-1], z[:, :, ::4, ::4, ::4])
        assert abs(float(z.double().abs().sum()) - float(ab[-1])) <= 1e-9 * float(ab[-1])
    # PLMS is not DDIM: a loop that ran DDIM cannot meet the 2e-2 bar of the PLMS golden
    d = ((g['S4_z_final'] - gd['z_final']).abs().max() / g['S4_z_final'].abs().max()).item()
    assert d > 4e-2, d
    assert gk['calls'].tolist() == g['S4_calls'].tolist() == gs['calls'].tolist()
    assert gk['keep'].tolist() == [1, 3] and tuple(gk['z_final'].shape) == (4, 3, 16, 16, 16)
    assert torch.equal(gk['img_first'], load_golden('ddim_keep_tiny')['img_first'])              # the same blend before iteration 0
    assert tuple(gs['z'].shape) == (8, 3, 16, 16, 16) and tuple(gs['shapes'].shape) == (8, 1, 16, 16, 16)
    ts = ShapeSchedule(4).timesteps
    assert sorted(set(gk['calls'].tolist()), reverse=True) == [int(t) for t in ts]


# ------------------------------------------------------------------------------------------------ C ABI
def test_plms_struct_matches_header(L, tmp_path):
    """sizeof() and every field offset of es_plms_args as the C compiler sees them == the ctypes mirror; the new union member is not
    the largest, so es_op (and the model-file format) keeps its size; the op kinds are 23..25 (22 stays unassigned, as 20); ABI still 10."""
    from echoscene_amd import hip
    fields = [n for n, _ in hip.PlmsArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "echoscene_hip.h"\nint main(){' + \
        'printf("size %zu\\n", sizeof(es_plms_args)); printf("op %zu\\n", sizeof(es_op));' + \
        ''.join('printf("%s %%zu\\n", offsetof(es_plms_args, %s));' % (n, n) for n in fields) + \
        'printf("kinds %d\\n", ES_OP_PLMS * 10000 + ES_OP_PLMS_FIRST_A * 100 + ES_OP_PLMS_FIRST_B);return 0;}'
    c = tmp_path / 'plms.c'
    c.write_text(src)
    exe = tmp_path / 'plms'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    vals = dict(zip(out[0::2], map(int, out[1::2])))
    assert vals['size'] == C.sizeof(hip.PlmsArgs) == 72
    assert vals['op'] == C.sizeof(hip.Op)
    for n in fields:
        assert vals[n] == getattr(hip.PlmsArgs, n).offset, n
    assert vals['kinds'] == 232425 and (hip.OP_PLMS, hip.OP_PLMS_FIRST_A, hip.OP_PLMS_FIRST_B) == (23, 24, 25)
    assert C.sizeof(hip.PlmsArgs) < C.sizeof(hip.LinearArgs) <= C.sizeof(hip.Op) - 8
    assert C.sizeof(hip.UpdateArgs) == 80 and L.es_abi_version() == 10


def test_plms_symbols_and_pointer_tables(L):
    from echoscene_amd import hip
    for name in ('es_plms_update', 'es_plms_first_a', 'es_plms_first_b'):
        assert name in hip.EXPORTS and getattr(L, name) is not None
    u_off = hip.Op.u.offset
    buf = (C.c_size_t * 64)()
    want = sorted(u_off + getattr(hip.PlmsArgs, n).offset for n, typ in hip.PlmsArgs._fields_ if typ is C.c_void_p)
    for kind in (hip.OP_PLMS, hip.OP_PLMS_FIRST_A, hip.OP_PLMS_FIRST_B):
        n = L.es_op_pointer_offsets(kind, buf, 64)
        assert n == len(want) == 6 and sorted(buf[i] for i in range(n)) == want
    assert all(L.es_op_pointer_offsets(k, buf, 64) == -1 for k in (20, 22, 26))
    hdr = open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read()
    assert 'typedef struct es_plms_args' in hdr and 'ES_OP_PLMS = 23' in hdr


def test_plms_launchers_refuse_bad_arguments_on_the_host(L):
    """every pointer, the size, the strides and the alignment are checked before anything is enqueued (no device needed)"""
    from echoscene_amd import hip

    def good():
        a = hip.PlmsArgs()
        a.x = a.eps = a.coef = a.step = a.ring = a.xsave = 4096
        a.n, a.coef_stride, a.ring_stride = 12288, 4, 12288
        return a
    for fn, name, first in ((L.es_plms_update, b'es_plms_update', False), (L.es_plms_first_a, b'es_plms_first_a', True),
                            (L.es_plms_first_b, b'es_plms_first_b', True)):
        assert fn(C.byref(hip.PlmsArgs()), None) != 0 and name in L.es_last_error()
        for field in ('x', 'eps', 'coef', 'step', 'ring') + (('xsave',) if first else ()):
            a = good()
            setattr(a, field, None)
            assert fn(C.byref(a), None) != 0 and b'NULL' in L.es_last_error(), field
        for field, v in (('n', 12286), ('n', 0), ('coef_stride', 3), ('ring_stride', 12284), ('ring_stride', 12290)):
            a = good()
            setattr(a, field, v)
            assert fn(C.byref(a), None) != 0 and name in L.es_last_error(), (field, v)
        a = good()
        a.eps_nslab, a.eps_slab_stride = 2, 12290
        assert fn(C.byref(a), None) != 0 and b'eps_slab_stride' in L.es_last_error()
        for field in ('x', 'eps', 'ring'):
            a = good()
            setattr(a, field, 4096 + 8)
            assert fn(C.byref(a), None) != 0 and b'aligned' in L.es_last_error(), field


# ------------------------------------------------------------------------------------------------ the public interface
def test_signatures_take_the_sampler_keywords():
    from echoscene_amd.model import scene
    from echoscene_amd.samplers import ShapeDenoiser, sample_layout_and_shape
    for fn in (scene.Sg2ScDiffModel.sample, scene.Sg2ScDiffModel.sample_with_changes, scene.Sg2ScDiffModel.sample_with_additions,
               scene.EchoToShape.rel2shape):
        ps = inspect.signature(fn).parameters
        for k in ('shape_sampler', 'shape_steps'):
            assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None, (fn.__name__, k)
    assert inspect.signature(ShapeDenoiser.__init__).parameters['sampler'].default == 'ddim'
    assert inspect.signature(ShapeDenoiser.sample).parameters['sampler'].default is None
    assert inspect.signature(sample_layout_and_shape).parameters['shape_sampler'].default is None


def _scene_model(typ):
    from echoscene_amd import synth, config as escfg
    from model.SGDiff import SGDiff
    return SGDiff(typ, escfg.tiny_diff_opt('cpu'), synth.VOCAB, replace_latent=False, with_changes=True, residual=True,
                  gconv_pooling='avg', with_angles=True, clip=True, separated=False)


def test_sampler_keyword_validation_without_a_device():
    """an 'echolayout' model refuses the keywords on all three calls (before any device work); the model's defaults are DDIM with 100
    steps; an unknown sampler or a non-positive step count is a ValueError before a denoiser is built"""
    ml = _scene_model('echolayout')
    a = (None, None, None, None)
    for kw in (dict(shape_sampler='plms'), dict(shape_steps=50), dict(shape_sampler='ddim', shape_steps=4)):
        with pytest.raises(ValueError, match='shape_sampler'):
            ml.sample_box_and_shape(*a, **kw)
        with pytest.raises(ValueError, match='shape_sampler'):
            ml.sample_boxes_and_shape_with_changes(*a, *a, [1], **kw)
        with pytest.raises(ValueError, match='shape_sampler'):
            ml.sample_boxes_and_shape_with_additions(*a, *a, [1], **kw)
    m = _scene_model('echoscene')
    S = m.diff.ShapeDiff
    assert S.shape_sampler == 'ddim' and S.ddim_steps == 100
    with pytest.raises(ValueError, match='shape_sampler'):
        S._denoiser(0.0, 'euler', None)
    with pytest.raises(ValueError, match='shape_steps'):
        S._denoiser(0.0, 'plms', 0)


# ------------------------------------------------------------------------------------------------ the shard protocol under gloo
class _CountingShard:
    """Toy backend of the shard protocol with the PLMS extension (no networks): counts what the loop asks of it.  Every object's state
    moves by the mean of ALL objects' codes; the second pass of iteration 0 moves it once more."""

    def __init__(self, O, rank, world, plms):
        from echoscene_amd.parallel import partition
        self.lo, self.hi, self.block = partition(O, world, rank)
        self.x = torch.arange(O, dtype=torch.float32)[self.lo:self.hi, None, None, None, None].repeat(1, 1, 1, 1, 2) + 1.0
        self.plms = plms
        self.trace = []

    def passes(self, i):
        return 2 if (self.plms and i == 0) else 1

    def codes_local(self, i, p=0):
        self.trace.append(('codes', i, p))
        return self.x.reshape(self.hi - self.lo, 2)[:, :1].repeat(1, 64) * (i + 1 + 10 * p)

    def step(self, i, codes_all, p=0):
        self.trace.append(('step', i, p))
        self.x = self.x + codes_all.mean()

    def latents_local(self):
        return self.x


def _worker_plms(rank, world, port, out, O, steps):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import echoscene_amd.parallel as par
    n = {'codes': 0, 'all': 0}
    orig = dist.all_gather_into_tensor

    def counting(o, i, group=None, **kw):
        n['all'] += 1
        n['codes'] += 1 if tuple(i.shape[1:]) == (64,) else 0
        return orig(o, i, group=group, **kw)
    dist.all_gather_into_tensor = counting
    sh = _CountingShard(O, rank, world, plms=True)
    z = par.sharded_ddim_loop(sh, O, steps, world)
    dist.all_gather_into_tensor = orig
    torch.save(dict(z=z, n=n, trace=sh.trace, own=sh.hi - sh.lo), out % rank)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('world,O', [(2, 4), (3, 2)])
def test_sharded_plms_loop_joins_s_plus_1_all_gathers_on_every_rank(tmp_path, world, O):
    """S iterations of a PLMS backend are S + 1 (stem -> all-gather -> rest) passes: every rank -- with O = 2 over 3 ranks also the
    one that owns no object -- joins S + 1 code all-gathers (+ the final latent gather) and gets the 1-rank result bit for bit; the
    second pass of iteration 0 is announced as pass 1; a backend without ``passes`` (DDIM) keeps one pass per iteration."""
    from echoscene_amd.parallel import sharded_ddim_loop, partition
    S = 4
    out = str(tmp_path / 'z%d.pt')
    port = 35500 + (os.getpid() % 2000) + world
    mp.spawn(_worker_plms, args=(world, port, out, O, S), nprocs=world, join=True)
    ref = _CountingShard(O, 0, 1, plms=True)
    z1 = sharded_ddim_loop(ref, O, S, 1)
    want = [(k, i, p) for i, p in [(0, 0), (0, 1)] + [(i, 0) for i in range(1, S)] for k in ('codes', 'step')]
    assert ref.trace == want
    owns = []
    for r in range(world):
        got = torch.load(out % r)
        assert got['n'] == {'codes': S + 1, 'all': S + 2}, (r, got['n'])
        assert got['trace'] == want, r
        assert torch.equal(got['z'], z1), r
        owns.append(got['own'])
    assert owns == [partition(O, world, r)[1] - partition(O, world, r)[0] for r in range(world)]
    if O < world:
        assert owns[-1] == 0
    d = _CountingShard(O, 0, 1, plms=False)
    sharded_ddim_loop(d, O, S, 1)
    assert d.trace == [(k, i, 0) for i in range(S) for k in ('codes', 'step')]
    assert not torch.equal(d.x, ref.x)


# ------------------------------------------------------------------------------------------------ sub-plan composition
@pytest.mark.parametrize('sharded', [False, True])
@pytest.mark.parametrize('plms', [False, True])
@pytest.mark.parametrize('n_blend', [0, 1])
def test_sub_plans_are_slices_of_the_step(n_blend, plms, sharded):
    """samplers.compose_step_plans on plain integers for ops (no library, no device): the identities the GPU tests assert on the
    plans a ShapeDenoiser really runs (tests/test_hip_plms.py, tests/test_hip_keep.py, tests/test_hip_vol.py)."""
    from echoscene_amd.samplers import SUB_PLANS, compose_step_plans
    plan, split, n_eps_ops, A, B = list(range(11)), 4, 10, 100, 101      # 10 denoiser ops (the first: the blend, if any) + the sampler op
    p = compose_step_plans(plan, n_blend, split, n_eps_ops, A, B, plms=plms, sharded=sharded)
    assert set(p) == set(SUB_PLANS)
    assert p['plan'] == plan and p['eps_plan'] == plan[:-1]
    if sharded:
        stem, main = p['stem_plan'], p['main_plan']
        assert stem + main == plan and stem == plan[:split]
    else:
        assert p['stem_plan'] is None and p['main_plan'] is None
    if plms:
        assert p['first_plan'] == plan[:-1] + [A] + plan[n_blend:-1] + [B]
    else:
        assert p['first_plan'] is None
    if plms and sharded:
        assert p['stem2_plan'] == stem[n_blend:] and (p['stem2_plan'] is stem) == (n_blend == 0)
        assert p['main_a_plan'] == main[:-1] + [A] and p['main_b_plan'] == main[:-1] + [B]
        # the two passes of iteration 0 are the unsharded first plan, cut at the exchange
        assert stem + p['main_a_plan'] + p['stem2_plan'] + p['main_b_plan'] == p['first_plan']
    else:
        assert p['main_a_plan'] is None and p['stem2_plan'] is None and p['main_b_plan'] is None
    assert plan == list(range(11)), 'the step itself is not modified'
