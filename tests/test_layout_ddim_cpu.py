"""CPU-only checks of strided DDIM sampling of the layout loop: the schedule against the tables the reference's DDIMSampler built
(tests/golden/make_golden_layout_ddim.py), a test-local fp32 restatement of the loop against every golden (it pins the goldens and the
bar before any GPU run), the additions to the C ABI, the plan next to the default one, the iteration arithmetic of the fused call and
the argument errors of the public calls.  No device compute is called here."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden, seeded_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


def _rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 1, 2: the schedule
@pytest.mark.parametrize('eta,et', [(0.0, 'eta0'), (0.7, 'eta07')])
@pytest.mark.parametrize('S', [4, 5, 100])
def test_layout_ddim_schedule_equals_the_reference_tables(S, eta, et):
    """timesteps and every coefficient column of LayoutDdimSchedule, torch.equal to what DDIMSampler.make_schedule built on the layout
    model's alphas_cumprod (T = 1000) and to what p_sample_ddim forms from it; keep_tab = the layout schedule's q_sample factors at ts"""
    from echoscene_amd.schedules import LayoutSchedule, LayoutDdimSchedule
    g = load_golden('layout_ddim_tiny')
    k = lambda name: g['tab_S%d_%s_%s' % (S, et, name)]
    base = LayoutSchedule(1000)
    s = LayoutDdimSchedule(base, S, eta)
    ts = k('ddim_timesteps').numpy()
    n = len(ts)
    assert np.array_equal(s.ddim_timesteps, ts) and np.array_equal(s.timesteps, ts[::-1])
    assert n == S and tuple(s.coef.shape) == (n, 5) and s.coef.dtype == torch.float32
    order = torch.arange(n - 1, -1, -1)
    a, a_prev = k('ddim_alphas').float(), k('ddim_alphas_prev').float()          # (alphas_prev is a float64 array of fp32 values)
    assert torch.equal(a_prev.double(), k('ddim_alphas_prev').double())
    sig = k('ddim_sigmas').to(torch.float32)                                       # torch.full(param_shape, sigmas[index]) rounds it
    assert torch.equal(s.ddim_alphas, a) and torch.equal(s.ddim_alphas_prev, a_prev) and torch.equal(s.ddim_sigmas, sig)
    assert torch.equal(s.coef[:, 0], k('ddim_sqrt_one_minus_alphas').float()[order])
    assert torch.equal(s.coef[:, 1], a.sqrt()[order])                              # a_t.sqrt()
    assert torch.equal(s.coef[:, 2], a_prev.sqrt()[order])                         # a_prev.sqrt()
    assert torch.equal(s.coef[:, 3], (1. - a_prev - sig ** 2).sqrt()[order])       # (1. - a_prev - sigma_t**2).sqrt()
    assert torch.equal(s.coef[:, 4], sig[order])
    assert bool((sig == 0).all()) == (eta == 0.0)
    tsi = torch.from_numpy(s.timesteps.copy())
    assert torch.equal(s.keep_tab[:, 0], base.sqrt_alphas_cumprod[tsi]) and torch.equal(s.keep_tab[:, 1], base.sqrt_one_minus_alphas_cumprod[tsi])
    assert torch.equal(s.keep_tab[:, 0], g['sac1000'][tsi]) and torch.equal(s.keep_tab[:, 1], g['s1mac1000'][tsi])


def test_issue_figures_and_the_index_error():
    """At T = 1000, S = 4 calls the denoiser at t = 751, 501, 251, 1; S = 1000 fails the way the reference does; the iteration count is
    len(ts), not necessarily ``steps``; the refused combinations"""
    from echoscene_amd.schedules import LayoutSchedule, LayoutDdimSchedule, ShapeSchedule
    g = load_golden('layout_ddim_tiny')
    base = LayoutSchedule(1000)
    assert g['S4_calls'].tolist() == [751, 501, 251, 1] == LayoutDdimSchedule(base, 4).timesteps.tolist()
    assert g['S5_calls'].tolist() == LayoutDdimSchedule(base, 5).timesteps.tolist()
    assert g['S100_calls'].tolist() == LayoutDdimSchedule(base, 100).timesteps.tolist() == list(range(991, 0, -10))
    with pytest.raises(IndexError):
        LayoutDdimSchedule(base, 1000)
    with pytest.raises(IndexError):
        ShapeSchedule(1000)
    assert len(LayoutDdimSchedule(base, 150).timesteps) == 167              # c = 6: range(0, 1000, 6) has 167 entries, the last is 996
    assert len(LayoutDdimSchedule(LayoutSchedule(100), 4).timesteps) == 4
    with pytest.raises(ValueError, match='no reference arithmetic'):
        LayoutDdimSchedule(LayoutSchedule(1000, model_mean_type='x0'), 4)
    with pytest.raises(ValueError, match='no reference arithmetic'):
        LayoutDdimSchedule(base, 4, clip_denoised=True)
    # model_var_type plays no part
    assert torch.equal(LayoutDdimSchedule(LayoutSchedule(1000, model_var_type='fixedlarge'), 5, 0.7).coef, LayoutDdimSchedule(base, 5, 0.7).coef)


# ------------------------------------------------------------------------------------------------ 3: the loop, restated in fp32
def ddim_loop_fp32(sd, oe, triples, x_T, sched, draws=None, mask=None, x0=None, keep_noise=None, trace=None, seen=None):
    """DDIMSampler.ddim_sampling on the layout denoiser, restated: the oracle's UNet1D evaluation plus the three update lines of
    p_sample_ddim, the blend with q_sample in front of every evaluation when a mask is given (samplers/ddim.py:160-163)."""
    from oracle import echoscene_oracle as orc
    O = x_T.shape[0]
    x = x_T.clone()
    for i, t in enumerate(sched.timesteps.tolist()):
        c = sched.coef[i]
        if mask is not None:
            q = sched.keep_tab[i, 0] * x0 + sched.keep_tab[i, 1] * keep_noise[i]
            x = q * mask[:, None] + (1. - mask[:, None]) * x
        if seen is not None:
            seen.append(x.clone())
        e = orc.unet1d_forward(sd, x, oe, triples, torch.full((O,), int(t), dtype=torch.int64))
        px0 = (x - c[0] * e) / c[1]
        x = c[2] * px0 + c[3] * e
        if draws is not None:
            x = x + c[4] * draws[i]
        if trace is not None:
            trace.append(x.clone())
    return x


def _tiny_sd(mc=128, ctx=128, prefix='unet1d_tiny.'):
    from echoscene_amd import config as escfg
    from echoscene_amd.model.unet import UNet1DModel
    kw = dict(escfg.layout_denoiser_kwargs(mc))
    kw['concat_dim'] = kw['crossattn_dim'] = ctx
    return seeded_state_dict(UNet1DModel(**kw), prefix)


def _bar(got, ref, what):
    """the rows path's bar: atol 1e-4 + rtol 1e-4"""
    err = (got - ref).abs()
    print('%s: max abs err %.3e (ref scale %.3e), worst err / bar %.3f' % (
        what, err.max().item(), ref.abs().max().item(), (err / (1e-4 + 1e-4 * ref.abs())).max().item()))
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4), what


@pytest.fixture(scope='module')
def tiny_sd():
    return _tiny_sd()


@pytest.mark.parametrize('tag,S,eta', [('S4', 4, 0.0), ('S5', 5, 0.0), ('S4_eta07', 4, 0.7), ('S100', 100, 0.0)])
def test_fp32_restatement_meets_the_tiny_goldens(tiny_sd, tag, S, eta):
    from echoscene_amd.schedules import LayoutSchedule, LayoutDdimSchedule
    g = load_golden('layout_ddim_tiny')
    sched = LayoutDdimSchedule(LayoutSchedule(1000), S, eta)
    trace = []
    x = ddim_loop_fp32(tiny_sd, g['obj_embed'], g['triples'], g['noise'][0], sched, draws=g['noise'][1:] if eta else None, trace=trace)
    if S <= 5:
        for i in range(S):
            _bar(trace[i], g[tag + '_states'][i], '%s after iteration %d' % (tag, i))
        assert torch.equal(g[tag + '_states'][-1], g[tag + '_x_final'])
    _bar(x, g[tag + '_x_final'], tag + ' final')


def test_eta_changes_the_result_and_ddim_is_not_the_ancestral_loop():
    g = load_golden('layout_ddim_tiny')
    assert (g['S4_eta07_x_final'] - g['S4_x_final']).abs().max() > 1e-2
    assert not torch.equal(g['S4_states'][0], g['S5_states'][0])


@pytest.mark.slow
def test_fp32_restatement_meets_the_full_width_golden():
    from echoscene_amd.schedules import LayoutSchedule, LayoutDdimSchedule
    g, gf = load_golden('layout_ddim_full'), load_golden('unet1d_full')
    sd = _tiny_sd(512, 1280, 'unet1d_full.')
    sched = LayoutDdimSchedule(LayoutSchedule(1000), 10)
    trace = []
    x = ddim_loop_fp32(sd, gf['loop_obj_embed'], gf['loop_triples'], g['x_T'], sched, trace=trace)
    assert g['calls'].tolist() == sched.timesteps.tolist()
    _bar(trace[0], g['x_iter0'], 'full width after iteration 0')
    _bar(x, g['x_final'], 'full width, S = 10')


def test_fp32_restatement_meets_the_masked_golden(tiny_sd):
    from echoscene_amd.schedules import LayoutSchedule, LayoutDdimSchedule
    g = load_golden('layout_ddim_keep_tiny')
    keep = g['keep'].long()
    xs, qs = [int(v) for v in g['seeds']]
    x0 = torch.zeros(4, 8)
    x0[keep] = _rnd((len(keep), 8), xs, 0.5)
    table = torch.stack([_rnd((4, 8), qs + k) for k in range(4)])
    assert torch.equal(x0, g['x0']) and torch.equal(table, g['keep_noise'])
    mask = torch.zeros(4)
    mask[keep] = 1.0
    sched = LayoutDdimSchedule(LayoutSchedule(1000), 4)
    seen = []
    x = ddim_loop_fp32(tiny_sd, g['obj_embed'], g['triples'], g['x_T'], sched, mask=mask, x0=x0, keep_noise=table, seen=seen)
    _bar(seen[0], g['img_first'], 'blended state in front of iteration 0')
    _bar(x, g['x_final'], 'masked S = 4 final')
    gen = (mask == 0).nonzero().flatten()
    assert torch.equal(seen[0][gen], g['x_T'][gen])
    # the kept nodes are context: the generated rows of the masked golden differ from the unmasked run's
    assert float((g['x_final'][gen] - g['x_final_unmasked'][gen]).abs().amax(dim=1).min()) > 1e-3


def test_scene_golden_is_consistent():
    g, ge = load_golden('scene_layout_ddim_tiny'), load_golden('scene_e2e_tiny')
    assert torch.equal(g['objs'], ge['objs']) and torch.equal(g['triples'], ge['triples'])
    assert g['lay_calls'].tolist() == g['sc_calls'].tolist() == [76, 51, 26, 1]          # T = 100 of the tiny config, S = 4
    for fam in ('lay_', 'sc_'):
        assert tuple(g[fam + 'sizes'].shape) == (8, 3) and tuple(g[fam + 'angles'].shape) == (8, 2)
    assert not torch.equal(g['lay_sizes'], ge['echolayout_sizes'])


# ------------------------------------------------------------------------------------------------ 4: the C ABI
def test_struct_sizes_abi_and_the_new_op_code(L, tmp_path):
    from echoscene_amd import hip
    names = {'es_ddpm_keep_args': hip.DdpmKeepArgs, 'es_op': hip.Op, 'es_update_args': hip.UpdateArgs, 'es_linear_args': hip.LinearArgs,
             'es_plms_args': hip.PlmsArgs, 'es_blend_args': hip.BlendArgs}
    src = '#include <stdio.h>\n#include "echoscene_hip.h"\nint main(){' + ''.join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + 'printf("rows %d\\n", ES_OP_DDIM_ROWS);return 0;}'
    c = tmp_path / 'sz.c'
    c.write_text(src)
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    vals = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert vals[n] == C.sizeof(cls), '%s: C %d vs ctypes %d' % (n, vals[n], C.sizeof(cls))
    assert vals['rows'] == hip.OP_DDIM_ROWS and hip.OP_DDIM_ROWS > 25
    assert C.sizeof(hip.Op) == 488 and C.sizeof(hip.UpdateArgs) == 80 and L.es_abi_version() == 10
    hdr = open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read()
    raw = C.CDLL(hip.LIB_PATH)
    assert 'es_ddim_rows_update(' in hdr and 'es_ddim_rows_update' in hip.EXPORTS and hasattr(raw, 'es_ddim_rows_update')
    assert 'ES_OP_DDIM_ROWS = %d' % hip.OP_DDIM_ROWS in hdr
    # the model-file relocation of the new op: the nine pointer fields of es_ddpm_keep_args
    u_off = hip.Op.u.offset
    buf = (C.c_size_t * 64)()
    n = L.es_op_pointer_offsets(hip.OP_DDIM_ROWS, buf, 64)
    want = sorted(u_off + getattr(hip.DdpmKeepArgs, name).offset for name, typ in hip.DdpmKeepArgs._fields_ if typ is C.c_void_p)
    assert n == 9 == len(want) and sorted(buf[i] for i in range(n)) == want


def test_launcher_refuses_bad_arguments_on_the_host(L):
    """every check runs before anything is enqueued (no device needed)"""
    from echoscene_amd import hip
    fn = L.es_ddim_rows_update

    def good(masked=True, noise=True):
        a = hip.DdpmKeepArgs()
        a.x = a.eps = a.coef = a.step = 4096
        a.n, a.row, a.n_tab, a.coef_stride = 24, 8, 10, 5
        if noise:
            a.noise, a.noise_stride = 4096, 24
        if masked:
            a.x0 = a.mask = a.keep_noise = a.tab = 4096
            a.keep_noise_stride = 24
        return a
    assert fn(C.byref(hip.DdpmKeepArgs()), None) != 0 and b'es_ddim_rows_update' in L.es_last_error()
    for f in ('x', 'eps', 'coef', 'step'):
        a = good()
        setattr(a, f, None)
        assert fn(C.byref(a), None) != 0 and b'NULL' in L.es_last_error(), f
    for f in ('x0', 'mask', 'keep_noise', 'tab'):                    # the four go together
        a = good()
        setattr(a, f, None)
        assert fn(C.byref(a), None) != 0 and b'together' in L.es_last_error(), f
        a = good(masked=False)
        setattr(a, f, 4096)
        assert fn(C.byref(a), None) != 0 and b'together' in L.es_last_error(), f
    a = good()
    a.clip_x0 = 1
    assert fn(C.byref(a), None) != 0 and b'clip_x0' in L.es_last_error()
    for f, v in (('n', 20), ('n', 0), ('row', 0), ('n_tab', 0), ('coef_stride', 4), ('noise_stride', 16), ('keep_noise_stride', 16)):
        a = good()
        setattr(a, f, v)
        assert fn(C.byref(a), None) != 0 and b'es_ddim_rows_update' in L.es_last_error(), (f, v)
    a = good(noise=False)
    a.coef_stride = 3
    assert fn(C.byref(a), None) != 0
    a = good()
    a.eps_nslab, a.eps_slab_stride = 2, 16
    assert fn(C.byref(a), None) != 0


# ------------------------------------------------------------------------------------------------ 5: plans and arguments
def _dry_ops(sampler, keep=False, eta=0.0, O=8, S=4, T=100, mc=128):
    """samplers.emit_layout_step on a CPU Builder (tests/test_keep_boxes_cpu.py's dry_layout_ops, with the sampler argument)"""
    from echoscene_amd import synth, config as escfg
    from echoscene_amd.model.unet import UNet1DModel
    from echoscene_amd.plan import Builder, GraphIndex, UNet1DWeights
    from echoscene_amd.samplers import _cap, _cpu_sd, emit_layout_step
    from echoscene_amd.schedules import LayoutSchedule, LayoutDdimSchedule
    dev = torch.device('cpu')
    net = UNet1DModel(**escfg.layout_denoiser_kwargs(mc))
    synth.seeded_fill_(net, prefix='dry.')
    w = UNet1DWeights(_cpu_sd(net), net, dev)
    _, triples = synth.synthetic_graph(O, seed=3)
    g = GraphIndex(triples, O, dev, capacity=_cap(triples.shape[0]))
    sched = LayoutSchedule(T)
    if sampler == 'ddim':
        sched = LayoutDdimSchedule(sched, S, eta)
    n = len(sched.timesteps)
    b = Builder(dev)
    tables = dict(emb=None, emb_all=torch.zeros(n, w.emb_all.N), t_lin=torch.zeros(n, 64))
    emit_layout_step(b, w, g, torch.zeros(O, 640), torch.zeros(n, mc), tables, n, sched.coef, sched.keep_tab, keep=keep, sampler=sampler,
                     step_noise=sampler == 'ddpm' or eta != 0.0)
    return b.ops


def test_ddim_step_plan_is_the_default_plan_with_the_last_op_replaced(L):
    from echoscene_amd import hip
    from echoscene_amd.plan import count_launches
    from test_keep_boxes_cpu import layout_op_signature
    plain = _dry_ops('ddpm')
    sp = layout_op_signature(plain)
    for keep in (False, True):
        for eta in (0.0, 0.7):
            ops = _dry_ops('ddim', keep=keep, eta=eta)
            sd = layout_op_signature(ops)
            assert len(sd) == len(sp) and sd[:-1] == sp[:-1]
            assert sp[-1][0] == hip.OP_DDPM and sd[-1][0] == hip.OP_DDIM_ROWS
            a = ops[-1].u.keep
            assert (a.n, a.row, a.n_tab, a.coef_stride, a.inc_step, a.clip_x0) == (64, 8, 4, 5, 1, 0)
            assert bool(a.noise) == (eta != 0.0) and bool(a.mask) == bool(a.x0) == bool(a.keep_noise) == bool(a.tab) == keep
            assert a.eps_nslab == plain[-1].u.update.eps_nslab and a.eps_slab_stride == plain[-1].u.update.eps_slab_stride
            assert count_launches(ops) == count_launches(plain)           # one launch, as the ancestral update
    for n, extra in ((4096, 0), (4104, 1)):
        o = hip.Op()
        o.kind = hip.OP_DDIM_ROWS
        o.u.keep.n, o.u.keep.inc_step = n, 1
        assert count_launches([o]) == 1 + extra
    from echoscene_amd.samplers import emit_layout_step
    with pytest.raises(ValueError):
        emit_layout_step(None, None, None, None, None, None, 4, sampler='euler')
    with pytest.raises(ValueError, match='clip_denoised'):
        emit_layout_step(None, None, None, None, None, None, 4, clip=True, sampler='ddim')


@pytest.mark.parametrize('lay,shp,first,want', [(100, 100, 0, (1, 0)), (100, 50, 1, (2, 2)), (8, 4, 0, (2, 0)), (2, 4, 0, (0, 2))])
def test_iteration_arithmetic_of_the_fused_call(lay, shp, first, want):
    """(layout, shape) iterations -> (layout steps per fused replay, layout steps left over): (100, 50 + PLMS) fuses 2 per replay over
    the 49 steady shape iterations and leaves 2; (2, 4): r = 0, nothing fused, the whole layout loop runs by itself"""
    from echoscene_amd.samplers import fused_iterations
    r, left = fused_iterations(lay, shp, first)
    assert (r, left) == want
    assert r * (shp - first) * (r >= 1) + left == lay


def test_signatures_take_the_layout_keywords():
    from echoscene_amd.model import scene
    from echoscene_amd.samplers import LayoutDenoiser, emit_layout_step
    for fn in (scene.Sg2ScDiffModel.sample, scene.Sg2ScDiffModel.sample_with_changes, scene.Sg2ScDiffModel.sample_with_additions,
               scene.Sg2BoxDiffModel.sampleBoxes, scene.Sg2BoxDiffModel.sampleBoxes_with_changes,
               scene.Sg2BoxDiffModel.sampleBoxes_with_additions, scene.EchoToLayout.generate_layout_sg):
        ps = inspect.signature(fn).parameters
        for k in ('layout_sampler', 'layout_steps', 'layout_eta'):
            assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None, (fn.__name__, k)
    ps = inspect.signature(LayoutDenoiser.__init__).parameters
    assert (ps['sampler'].default, ps['steps'].default, ps['eta'].default, ps['weights'].default) == ('ddpm', None, 0.0, None)
    assert inspect.signature(emit_layout_step).parameters['sampler'].default == 'ddpm'


def _scene_model(typ, **layout_kw):
    from echoscene_amd import synth, config as escfg
    from model.SGDiff import SGDiff
    opt = escfg.tiny_diff_opt('cpu')
    for k, v in layout_kw.items():
        opt.layout_branch.diffusion_kwargs[k] = v
    return SGDiff(typ, opt, synth.VOCAB, replace_latent=False, with_changes=True, residual=True,
                  gconv_pooling='avg', with_angles=True, clip=True, separated=False)


@pytest.mark.parametrize('typ', ['echolayout', 'echoscene'])
def test_layout_keyword_validation_without_a_device(typ):
    """an unknown sampler, layout_steps / layout_eta with 'ddpm' (or without a sampler: the default is 'ddpm'), 'ddim' without a step
    count: ValueError on all three calls of both model types before any device work; the defaults"""
    m = _scene_model(typ)
    Ld = m.diff.LayoutDiff
    assert (Ld.layout_sampler, Ld.layout_steps) == ('ddpm', None)
    a = (None, None, None, None)
    for kw in (dict(layout_sampler='euler'), dict(layout_steps=10), dict(layout_eta=0.5), dict(layout_sampler='ddpm', layout_steps=10),
               dict(layout_sampler='ddpm', layout_eta=0.3), dict(layout_sampler='ddim'), dict(layout_sampler='ddim', layout_steps=0)):
        with pytest.raises(ValueError, match='layout_'):
            m.sample_box_and_shape(*a, **kw)
        with pytest.raises(ValueError, match='layout_'):
            m.sample_boxes_and_shape_with_changes(*a, *a, [1], **kw)
        with pytest.raises(ValueError, match='layout_'):
            m.sample_boxes_and_shape_with_additions(*a, *a, [1], **kw)
    assert Ld.layout_options() == ('ddpm', None, 0.0)
    assert Ld.layout_options('ddim', 4) == ('ddim', 4, 0.0) and Ld.layout_options('ddim', 4, 0.7) == ('ddim', 4, 0.7)
    assert Ld.layout_options('ddpm', None, 0.0) == ('ddpm', None, 0.0)
    Ld.layout_sampler, Ld.layout_steps = 'ddim', 10                 # the attributes are the defaults of the keywords
    assert Ld.layout_options() == ('ddim', 10, 0.0) and Ld.layout_options(steps=5) == ('ddim', 5, 0.0)
    assert Ld.layout_options('ddpm') == ('ddpm', None, 0.0)


def test_x0_predicting_models_refuse_ddim():
    m = _scene_model('echolayout', model_mean_type='x0')
    with pytest.raises(ValueError, match='no reference arithmetic'):
        m.sample_box_and_shape(None, None, None, None, layout_sampler='ddim', layout_steps=4)
    from echoscene_amd.samplers import LayoutDenoiser
    with pytest.raises(ValueError, match='layout_steps'):
        LayoutDenoiser(None, {}, torch.device('cpu'), sampler='ddpm', steps=4)
    with pytest.raises(ValueError, match='layout_sampler'):
        LayoutDenoiser(None, {}, torch.device('cpu'), sampler='plms')
    with pytest.raises(ValueError, match='no reference arithmetic'):
        LayoutDenoiser(None, dict(model_mean_type='x0'), torch.device('cpu'), sampler='ddim', steps=4)
