#!/usr/bin/env python
"""Scene calls over a sequence of scene sizes through the drop-in API (the reference's eval loop walks scenes of different
object counts): first call at a new size (plan build + graph capture) against the repeated call.
usage: python tools/scene_sizes_latency.py [sizes, default 32,10,16,10,6,16] [--shape-sampler ddim|plms] [--shape-steps K] [--layout-sampler ddpm|ddim] [--layout-steps K] [--repeats N] [--alternate]
(--shape-sampler / --shape-steps / --layout-sampler / --layout-steps: the keywords of the same names of sample_box_and_shape;
--repeats: calls per size, default 2)"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from echoscene_amd import synth, config as escfg
from model.SGDiff import SGDiff

import argparse
ap = argparse.ArgumentParser()
ap.add_argument('sizes', nargs='?', default='32,10,16,10,6,16')
ap.add_argument('--shape-sampler', default=None)
ap.add_argument('--shape-steps', type=int, default=None)
ap.add_argument('--layout-sampler', default=None)
ap.add_argument('--layout-steps', type=int, default=None)
ap.add_argument('--repeats', type=int, default=2)
ap.add_argument('--alternate', action='store_true', help='after each size also make the default call: both denoisers resident')
cli = ap.parse_args()
sizes = [int(x) for x in cli.sizes.split(',')]
skw = {k: v for k, v in (('shape_sampler', cli.shape_sampler), ('shape_steps', cli.shape_steps), ('layout_sampler', cli.layout_sampler),
                          ('layout_steps', cli.layout_steps)) if v is not None}
opt = escfg.default_diff_opt('cuda', concat=False)
m = SGDiff('echoscene', opt, synth.VOCAB, replace_latent=False, with_changes=True, residual=True, gconv_pooling='avg',
           with_angles=True, clip=True, separated=False)
synth.seeded_fill_(torch.nn.Module.state_dict(m.diff), prefix='lat.diff.')
synth.seeded_fill_(m.diff.ShapeDiff.df, prefix='lat.df.')
synth.seeded_fill_(m.diff.ShapeDiff.vqvae, prefix='lat.vq.')
m.diff.optimizer_ini()
m.cuda()
m.eval()
for k, O in enumerate(sizes):
    objs, triples = synth.synthetic_graph(O, seed=20 + k)
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=20 + k)
    args = (objs.cuda(), triples.cuda(), tf.cuda(), rf.cuda())
    ts = []
    for i in range(max(2, cli.repeats)):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        d = m.sample_box_and_shape(*args, gen_shape=True, **skw)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print('O = %2d (T = %3d)%s: first call %.3f s, repeated %.3f s, finite %s' % (
          O, triples.shape[0], ''.join(' %s=%s' % kv for kv in skw.items()), ts[0], min(ts[1:]),
          bool(torch.isfinite(d['shapes']).all())), flush=True)
    print('        device memory: %.2f GB allocated now, %.2f GB peak' % (torch.cuda.memory_allocated() / 2 ** 30,
          torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
    if cli.alternate and skw:
        m.sample_box_and_shape(*args, gen_shape=True)
        torch.cuda.synchronize()
        print('        after the default call as well: %.2f GB allocated now, %.2f GB peak' % (torch.cuda.memory_allocated() / 2 ** 30,
              torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
