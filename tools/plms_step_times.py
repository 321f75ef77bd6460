#!/usr/bin/env python
"""ms per steady PLMS iteration against ms per DDIM iteration of the same build: the bench's shape denoiser (model_channels 224,
100-step schedule), one ShapeDenoiser, both plans replayed as captured graphs, repetitions interleaved (DDIM, PLMS, DDIM, ...).
The only difference between the two plans is their last op (es_ddim_update / es_plms_update).
usage: python tools/plms_step_times.py [--objects 32] [--steps 20] [--reps 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from echoscene_amd import synth, config as escfg                       # noqa: E402
from echoscene_amd.model.unet import DiffusionUNet                     # noqa: E402
from echoscene_amd.samplers import ShapeDenoiser                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--objects', type=int, default=32)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--reps', type=int, default=5)
a = ap.parse_args()
dev = torch.device('cuda')
conf = escfg.shape_df_conf(224)
df = DiffusionUNet(conf.unet.params, conditioning_key='crossattn')
synth.seeded_fill_(df, prefix='bench.shape.')
den = ShapeDenoiser(df, conf.model.params, ddim_steps=100, device=dev)
O = a.objects
objs, triples = synth.synthetic_graph(O, seed=5)
uc = torch.randn(O, 1, 1280, generator=torch.Generator().manual_seed(6))
noise1 = synth.shape_noise(seed=7)
plans = {}
for name in ('ddim', 'plms'):
    den.sample(uc, triples, noise1, n_steps=3, sampler=name)          # builds the plan, captures its graphs
    plans[name] = den._plan_for(uc, triples, None, sampler=name)
torch.cuda.synchronize()
ms = {'ddim': [], 'plms': []}
for _ in range(a.reps):
    for name, st in plans.items():
        st['x'].copy_(noise1.to(dev).expand(O, *den.z_shape))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st['plan'].sample(st['step'], 1, a.steps, use_graph=True)      # iterations 1 .. steps: the steady plan of either sampler
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / a.steps)
for name in ms:
    xs = sorted(ms[name])
    print('%s: ms per iteration median %.3f min %.3f max %.3f (%d reps x %d iterations, O = %d)'
          % (name, xs[len(xs) // 2], xs[0], xs[-1], a.reps, a.steps, O))
d, p = sorted(ms['ddim'])[a.reps // 2], sorted(ms['plms'])[a.reps // 2]
print('plms / ddim = %.4f' % (p / d))
