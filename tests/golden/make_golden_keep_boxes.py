#!/usr/bin/env python
"""Golden vectors of box-preserving sampling (the masked ancestral layout loop), from the REFERENCE ITSELF (read-only).

    python tests/golden/make_golden_keep_boxes.py --ref <checkout of the reference> [--only NAME]
    python tests/golden/make_golden_keep_boxes.py --only plan_ops        (no reference needed; run ON THE PARENT COMMIT, see below)

Loads make_golden.py for its helpers (reference import with stand-ins, seeded fill, save) and stores numbers only.

The reference's layout ``GaussianDiffusion`` has no masked loop.  ``masked_loop`` below is the loop of ``p_sample_loop_sg``
(diffusion_ddpm.py:330-345) with the blend of ``DDIMSampler.ddim_sampling`` (samplers/ddim.py:160-163) in front of every step: a few
lines of this file around the reference's own ``p_sample_sg`` and ``q_sample``, with q_sample's draws injected.

  layout_keep_tiny: the network, graph and noise of layout_loop_tiny (tiny width, O = 8, T = 100); nodes ``keep`` kept at ``x0``;
      x_final / x_final_clip (clip_denoised=True), the state the denoiser sees at iterations 0 and 99, and the reference's
      sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod for T = 100 and T = 1000.  The generator ASSERTS that every generated row
      differs from the unmasked golden by more than ten times the loop test's bar (the kept nodes really are context).
  box_pre: ``scale_box_params`` (6 and 7 columns, one box at a time as the reference handles them, float64 in / rounded once) with the
      statistics of the box_post fixture, and ``preprocess_angle2sincos``.
  scene_keep_boxes_tiny: the scene calls of scene_e2e_tiny / scene_edit_tiny with the layout loop replaced by ``masked_loop``:
      'echolayout' sample_box_and_shape and 'echoscene' sample_boxes_and_shape_with_changes.
  plan_ops -> layout_plan_ops_tiny.json: the op list of the UNMASKED layout step as tests/test_keep_boxes_cpu.py's dry_layout_ops emits
      it, recorded on the commit BEFORE this feature (copy this file and that test file into a checkout of it).
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden', os.path.join(HERE, 'make_golden.py'))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)
synth, escfg, fill, rnd, save = mg.synth, mg.escfg, mg.fill, mg.rnd, mg.save

KEEP = [0, 3, 6]                       # kept nodes of layout_keep_tiny (O = 8)
X0_SEED, QNOISE_SEED = 71, 1950
SCENE_KEEP = [0, 2, 5, 6]              # kept nodes of scene_keep_boxes_tiny (O = 8)
SCENE_X0_SEED, SCENE_QNOISE_SEED = 73, 1970
BAR = 2e-4                             # atol of test_layout_loop_tiny_100_steps_vs_reference_golden


def masked_loop(x0, keep, table, seen=None):
    """p_sample_loop_sg with the kept rows replaced by q_sample(x0, t, table[i]) in front of the denoiser of iteration i, and by x0
    after the last one.  ``x0`` [O, 8] (rows outside ``keep`` unused), ``table`` [T, O, 8]."""
    def loop(self, denoise_fn, shape, device, obj_embed, triples, condition, noise_fn=torch.randn, clip_denoised=True,
             keep_running=False):
        x_t = noise_fn(size=shape, dtype=torch.float, device=device)
        for i, t in enumerate(reversed(range(self.num_timesteps))):
            t_ = torch.empty(shape[0], dtype=torch.int64, device=device).fill_(t)
            x_t = x_t.clone()
            x_t[keep] = self.q_sample(x0, t_, noise=table[i])[keep]
            if seen is not None:
                seen.append(x_t.clone())
            x_t = self.p_sample_sg(denoise_fn=denoise_fn, data=x_t, t=t_, obj_embed=obj_embed, triples=triples, condition=condition,
                                   noise_fn=noise_fn, clip_denoised=clip_denoised, return_pred_xstart=False)
        x_t = x_t.clone()
        x_t[keep] = x0[keep]
        return x_t
    return loop


def case_layout_keep_tiny():
    import model.networks.diffusion_layout.diffusion_ddpm as dd
    from model.networks.diffusion_layout.diffusion_ddpm import DiffusionPoint, GaussianDiffusion, get_betas
    net, kw = mg._unet1d(128, 128)
    fill(net, 'unet1d_tiny.')
    O, T = 8, 100
    noise = synth.layout_noise(O, 8, T, seed=7)
    df = DiffusionPoint(denoise_net=net, config=escfg.AttrDict(angle_dim=2), **dict(escfg.layout_diffusion_kwargs(T)))
    objs, triples = synth.synthetic_graph(O, seed=3)
    oe = rnd((O, 640), 100 + 3)
    plain = np.load(os.path.join(HERE, 'layout_loop_tiny.npz'))
    assert np.array_equal(plain['obj_embed'], oe.numpy()) and np.array_equal(plain['triples'], triples.numpy())
    x0 = torch.zeros(O, 8)
    x0[KEEP] = rnd((len(KEEP), 8), X0_SEED, 0.5)
    table = torch.stack([rnd((O, 8), QNOISE_SEED + k) for k in range(T)])
    out = {}
    _orig = GaussianDiffusion.p_sample_loop_sg
    for tag, clip in (('', False), ('_clip', True)):
        calls = {'n': 0}

        def noise_fn(size, dtype, device):
            i = calls['n']
            calls['n'] += 1
            return noise[i].clone()
        seen = []
        GaussianDiffusion.p_sample_loop_sg = masked_loop(x0, KEEP, table, seen)
        try:
            with torch.no_grad():
                x = df.gen_samples_sg((O, 8), 'cpu', oe, triples, condition=None, noise_fn=noise_fn, clip_denoised=clip)
        finally:
            GaussianDiffusion.p_sample_loop_sg = _orig
        assert calls['n'] == T + 1 and len(seen) == T
        assert torch.equal(x[KEEP], x0[KEEP])
        out['x_final' + tag] = x
        if not clip:
            out['seen_first'], out['seen_last'] = seen[0], seen[-1]
    gen = [i for i in range(O) if i not in KEEP]
    ref = torch.from_numpy(plain['x_final'])
    d = (out['x_final'][gen] - ref[gen]).abs().amax(dim=1)
    print('layout_keep_tiny: per generated row, max |masked - unmasked| =', ['%.3e' % v for v in d.tolist()])
    assert float(d.min()) > 10 * BAR, 'the kept nodes do not act as context: choose other nodes / x0'
    dc = (out['x_final_clip'] - out['x_final'])[gen].abs().max().item()
    print('layout_keep_tiny: clip_denoised changes the generated rows by %.3e' % dc)
    assert dc > 10 * BAR
    gd = df.diffusion
    gd1000 = GaussianDiffusion(escfg.AttrDict(), get_betas('linear', 1e-4, 0.02, 1000), 'mse', 'eps', 'fixedsmall', True, False,
                               'obb', None)
    save('layout_keep_tiny', keep=np.array(KEEP), seeds=np.array([X0_SEED, QNOISE_SEED]), x0=x0,
         sac100=gd.sqrt_alphas_cumprod, s1mac100=gd.sqrt_one_minus_alphas_cumprod,
         sac1000=gd1000.sqrt_alphas_cumprod, s1mac1000=gd1000.sqrt_one_minus_alphas_cumprod, **out)


def case_box_pre():
    """the reference's own helpers/util.py scale_box_params / preprocess_angle2sincos"""
    import tempfile
    from helpers.util import scale_box_params, preprocess_angle2sincos
    stats = np.load(os.path.join(HERE, 'box_post.npz'))['stats']
    f = os.path.join(tempfile.mkdtemp(prefix='golden_box_'), 'stats.txt')
    np.savetxt(f, stats)
    assert np.array_equal(np.loadtxt(f), stats)
    rs = np.random.RandomState(1)
    lo = np.concatenate([stats[0:3], stats[6:9], stats[12:13]])
    hi = np.concatenate([stats[3:6], stats[9:12], stats[13:14]])
    boxes7 = (lo + (hi - lo) * rs.uniform(-0.1, 1.1, (33, 7))).astype(np.float32)        # metric, a little outside the range too
    boxes = boxes7[:, :6].copy()
    out = np.stack([scale_box_params(b.astype(np.float64), file=f) for b in boxes]).astype(np.float32)
    out7 = np.stack([scale_box_params(b.astype(np.float64), file=f, angle=True) for b in boxes7]).astype(np.float32)
    ang = torch.from_numpy(rs.uniform(-np.pi, np.pi, (33, 1)).astype(np.float32))
    sc = preprocess_angle2sincos(ang)
    save('box_pre', boxes=boxes, boxes_out=out, boxes7=boxes7, boxes7_out=out7, angle=ang, sincos=sc, stats=stats)


def case_scene_keep_boxes_tiny():
    import model.networks.diffusion_layout.diffusion_ddpm as dd
    out = {}
    O, T = 8, 100
    x0 = torch.zeros(O, 8)
    x0[SCENE_KEEP] = rnd((len(SCENE_KEEP), 8), SCENE_X0_SEED, 0.5)
    table = torch.stack([rnd((O, 8), SCENE_QNOISE_SEED + k) for k in range(T)])
    _orig = dd.GaussianDiffusion.p_sample_loop_sg
    dd.GaussianDiffusion.p_sample_loop_sg = masked_loop(x0, SCENE_KEEP, table)
    try:
        h = mg._SGDiffHarness('echolayout', False)
        d = h.call(lambda: h.m.sample_box_and_shape(h.objs, h.triples, h.tf, h.rf))
        for k in ('sizes', 'translations', 'angles'):
            out['lay_' + k] = d[k]
        out.update(objs=h.objs, triples=h.triples)
        h = mg._SGDiffHarness('echoscene', False)
        dec = (h.objs, h.triples, h.tf, h.rf)
        np.random.seed(5)
        keep, d = h.call(lambda: h.m.sample_boxes_and_shape_with_changes(*dec, *dec, [1], gen_shape=True))
        for k in ('sizes', 'translations', 'angles'):
            out['sc_chg_' + k] = d[k]
        out['sc_chg_keep'] = keep
    finally:
        dd.GaussianDiffusion.p_sample_loop_sg = _orig
    for fam in ('lay_', 'sc_chg_'):
        got = torch.cat([out[fam + k] for k in ('sizes', 'translations', 'angles')], 1)
        assert torch.equal(got[SCENE_KEEP], x0[SCENE_KEEP])
    save('scene_keep_boxes_tiny', keep=np.array(SCENE_KEEP), seeds=np.array([SCENE_X0_SEED, SCENE_QNOISE_SEED]), **out)


def case_plan_ops():
    sys.path.insert(0, os.path.dirname(HERE))
    import test_keep_boxes_cpu as t
    from echoscene_amd import hip
    from echoscene_amd.plan import Plan

    class _P:
        _arr = t.dry_layout_ops(keep=False)
    rec = dict(ops=t.layout_op_signature(_P._arr), n_launches=Plan.n_launches.fget(_P))
    assert not hasattr(hip, 'OP_DDPM_KEEP'), 'record the parent commit, not this tree'
    with open(os.path.join(HERE, 'layout_plan_ops_tiny.json'), 'w') as f:
        json.dump(rec, f)
    print('wrote layout_plan_ops_tiny.json: %d ops, %d launches' % (len(rec['ops']), rec['n_launches']))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None)
    ap.add_argument('--ref', default=None, help='checkout of the reference (read-only)')
    args = ap.parse_args()
    if args.only == 'plan_ops':
        case_plan_ops()
        sys.exit(0)
    if args.ref is None:
        ap.error('--ref is required for every case but plan_ops')
    mg.install_reference(args.ref)
    cases = dict(layout_keep_tiny=case_layout_keep_tiny, box_pre=case_box_pre, scene_keep_boxes_tiny=case_scene_keep_boxes_tiny)
    for name, fn in cases.items():
        if args.only in (None, name):
            fn()
