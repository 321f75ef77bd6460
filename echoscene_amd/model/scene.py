"""Host-side mirror of the reference's scene-level API:

    model/SGDiff.py       SGDiff                      (facade used by scripts/eval_3dfront.py:387-395,271)
    model/EchoScene.py    Sg2ScDiffModel              (layout + shape)
    model/EchoLayout.py   Sg2BoxDiffModel             (layout only)
    diffusion_layout/echo2layout.py  EchoToLayout     diffusion_shape/echo2shape.py  EchoToShape

Same constructor arguments, attribute names (=> same checkpoint keys), method
names, return structure and dtypes.  The arithmetic is NOT here: every method below prepares small
host-side index/concat glue and calls the HIP samplers (echoscene_amd/samplers.py); training
entry points raise NotImplementedError (out of scope).
"""
import os
import time

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from .. import config as escfg
from .params import _Holder, Emb, mlp
from .graph import GraphTripleConvNet
from .unet import UNet1DModel, DiffusionUNet
from .vqvae import VQVAE


def _dev(module):
    for p in module.parameters():
        return p.device
    return torch.device('cpu')


_BOX_OPTS = ('keep_box_nodes', 'keep_boxes', 'keep_box_noise')
_LAYOUT_OPTS = ('layout_sampler', 'layout_steps', 'layout_eta')
_COMPLETE_OPTS = ('complete_nodes', 'complete_sdfs', 'complete_ranges', 'complete_masks')


def _hip_device(d):
    if d.type != 'cuda':
        raise RuntimeError('the sampling path runs on the MI355X HIP library only: move the model to the GPU '
                           '(.cuda()) first -- there is no CPU fallback')
    return d


class DiffusionPoint(_Holder):
    """Key prefix holder: ``LayoutDiff.df.model.*`` (diffusion_layout/diffusion_ddpm.py:550-561)."""

    def __init__(self, denoise_net, diffusion_kwargs):
        super().__init__()
        self.model = denoise_net
        self.diffusion_kwargs = dict(diffusion_kwargs)


class EchoToLayout(nn.Module):
    def __init__(self, config, n_classes=None):
        super().__init__()
        lb = config.layout_branch
        if lb.denoiser != 'unet1d':
            raise NotImplementedError(lb.denoiser)
        # relation_condition (echo2layout.py:12,105): when true the reference hands the relation embeddings to the denoiser as `context`,
        # when false None -- and UNet1DModel.forward overwrites that argument with the GCN output ('crossattn', denoise_net.py:791-792)
        # or never reads it ('concat'): the flag has no effect on SAMPLING.  (Its only effect is in training, where false raises
        # NotImplementedError, echo2layout.py:93-96; training is out of scope here.)  Both values are accepted.
        self.rel_condition = bool(lb.get('relation_condition', True))
        self.df = DiffusionPoint(UNet1DModel(**lb.denoiser_kwargs), lb.diffusion_kwargs)
        self.config = config
        self.translation_dim = lb.get('translation_dim', 3)
        self.size_dim = lb.get('size_dim', 3)
        self.angle_dim = lb.angle_dim
        self.bbox_dim = self.translation_dim + self.size_dim + self.angle_dim
        self.trainable_params = list(self.df.parameters())
        self.scene_ids = None
        self.layout_sampler = 'ddpm'                    # 'ddim': the reference's DDIMSampler on a strided schedule of the trained timesteps
        self.layout_steps = None                        # ... of this many steps (needed with 'ddim')
        self.layout_eta = 0.0
        self._den, self._dens = None, {}

    def invalidate(self):
        self._den, self._dens = None, {}

    def set_input(self, data_dict):
        self.preds = data_dict['preds']
        self.rel = data_dict['c_b']
        self.uc_rel = data_dict['uc_b']

    def forward(self, *a, **k):
        raise NotImplementedError('training (EchoToLayout.forward / losses) is out of scope of this build')

    def layout_options(self, sampler=None, steps=None, eta=None):
        """``layout_sampler=`` / ``layout_steps=`` / ``layout_eta=`` of the sampling calls (None: the attributes of the same names)
        -> the validated (sampler, steps, eta).  No device work."""
        from ..schedules import LAYOUT_SAMPLERS
        sampler = self.layout_sampler if sampler is None else sampler
        if sampler not in LAYOUT_SAMPLERS:
            raise ValueError('layout_sampler must be one of %s, got %r' % (LAYOUT_SAMPLERS, sampler))
        if sampler == 'ddpm':
            if steps is not None or (eta is not None and float(eta) != 0.0):
                raise ValueError("layout_steps / layout_eta need layout_sampler='ddim' (the ancestral 'ddpm' loop runs every trained timestep)")
            return 'ddpm', None, 0.0
        steps = self.layout_steps if steps is None else steps
        eta = self.layout_eta if eta is None else eta
        if steps is None or int(steps) < 1:
            raise ValueError("layout_sampler='ddim' needs layout_steps, a positive step count; got %r" % (steps,))
        if self.df.diffusion_kwargs.get('model_mean_type', 'eps') != 'eps':
            raise ValueError("layout_sampler='ddim': model_mean_type=%r has no reference arithmetic under DDIM"
                             % (self.df.diffusion_kwargs.get('model_mean_type'),))
        return 'ddim', int(steps), float(eta)

    def _denoiser(self, sampler=None, steps=None, eta=None):
        """The default ('ddpm') denoiser lives in ``_den`` as it always has; another (sampler, steps, eta) gets a denoiser of its own -- its
        schedule, time tables and plans -- on the SAME packed weights; the two most recent of those stay resident."""
        sampler, steps, eta = self.layout_options(sampler, steps, eta)
        from ..samplers import LayoutDenoiser
        if sampler == 'ddpm':
            if self._den is None:
                w = next((d.w for d in self._dens.values()), None)
                self._den = LayoutDenoiser(self.df.model, self.df.diffusion_kwargs, _hip_device(_dev(self.df)), weights=w)
            return self._den
        key = (sampler, steps, eta)
        den = self._dens.get(key)
        if den is None:
            w = self._den.w if self._den is not None else next((d.w for d in self._dens.values()), None)
            den = LayoutDenoiser(self.df.model, self.df.diffusion_kwargs, _hip_device(_dev(self.df)), sampler=sampler, steps=steps,
                                 eta=eta, weights=w)
            while len(self._dens) >= 2:
                self._dens.pop(next(iter(self._dens)))
            self._dens[key] = den
        return den

    @torch.no_grad()
    def generate_layout_sg(self, box_dim, text=None, ret_traj=False, ddim=False, clip_denoised=False,
                           batch_seeds=None, noise=None, x0=None, mask=None, keep_noise=None, *, layout_sampler=None,
                           layout_steps=None, layout_eta=None):
        """echo2layout.py:112-126.  ``noise`` (optional, f32[T+1,O,box_dim]) makes the run reproducible.
        ``clip_denoised`` reaches the loop (gen_samples_sg, echo2layout.py:108; diffusion_ddpm.py:243-244).  ``ret_traj``, ``ddim``,
        ``text`` and ``batch_seeds`` are accepted and -- exactly as in the reference, whose ``sample`` (echo2layout.py:102-110)
        passes none of them on -- have no effect.  ``x0`` / ``mask`` / ``keep_noise``: the masked loop (LayoutDenoiser.sample).
        ``layout_sampler`` / ``layout_steps`` / ``layout_eta`` (keyword-only): see layout_options; ``noise`` is then
        f32[n_iter+1,O,box_dim] over the strided schedule's iterations."""
        return self.split_boxes(self._denoiser(layout_sampler, layout_steps, layout_eta).sample(self.uc_rel, self.preds, noise=noise, clip_denoised=bool(clip_denoised),
                                                        x0=x0, mask=mask, keep_noise=keep_noise))

    def split_boxes(self, x):
        """loop state [O, bbox_dim] -> its sizes | translations | angles columns"""
        s, t = self.size_dim, self.translation_dim
        return {'sizes': x[:, 0:s].contiguous(), 'translations': x[:, s:s + t].contiguous(),
                'angles': x[:, s + t:self.bbox_dim].contiguous()}


class EchoToShape(object):
    """Plain object, *not* an nn.Module, exactly like the reference: its
    networks are checkpointed under 'shape_df' / 'vqvae' and are not reached by ``SGDiff.cuda()``."""

    def __init__(self, opt):
        self.opt = opt
        self.isTrain = opt.hyper.isTrain
        self.device = opt.hyper.device
        df_conf = escfg.resolve_nested(opt.shape_branch.df_cfg)
        vq_conf = escfg.resolve_nested(opt.shape_branch.vq_cfg)
        dd = vq_conf.model.params.ddconfig
        z_sp = dd.resolution // (2 ** (len(dd.ch_mult) - 1))
        self.z_shape = (dd.z_channels, z_sp, z_sp, z_sp)
        self.df_conf = df_conf
        self.df = DiffusionUNet(df_conf.unet.params, conditioning_key=df_conf.model.params.conditioning_key)
        mp = vq_conf.model.params
        self.vqvae = VQVAE(dict(mp.ddconfig), mp.n_embed, mp.embed_dim)
        ck = opt.shape_branch.get('vq_ckpt', None)
        if ck is not None and os.path.exists(str(ck)):
            sd = torch.load(ck, map_location='cpu')
            self.vqvae.load_state_dict(sd['vqvae'] if 'vqvae' in sd else sd)
        self.df.to(self.device)
        self.vqvae.to(self.device)
        self.df_module, self.vqvae_module = self.df, self.vqvae
        self.trainable_params = list(self.df.parameters())
        self.ddim_steps = 100                           # hard-coded by the reference (echo2shape.py:118)
        if opt.misc.get('debug', 0) == 1:
            self.ddim_steps = 7
        self.shape_sampler = 'ddim'                     # 'plms': the reference's PLMSSampler (samplers/plms.py) on the same schedule
        self.uc_scale = 3.0                             # read but never applied (ddim.py:207-228)
        self._den = None
        self._dens = {}
        self._dec = None
        self.triples = None

    def invalidate(self):
        self._den = None
        self._dens = {}
        self._dec = None
        self._enc = None

    def set_input(self, input=None):
        self.rel = input['c_s']
        self.uc_rel = input['uc_s']
        self.triples = input.get('triples', None)

    def switch_eval(self):
        self.df.eval()
        self.vqvae.eval()

    def forward(self, *a, **k):
        raise NotImplementedError('training (EchoToShape.forward / p_losses) is out of scope of this build')

    def _denoiser(self, ddim_eta=0.0, sampler=None, steps=None):
        """``sampler`` / ``steps``: ``shape_sampler=`` / ``shape_steps=`` of the sampling calls (None: the attributes ``shape_sampler`` /
        ``ddim_steps``).  The default combination lives in ``_den`` as it always has; another (sampler, step count) gets a denoiser of
        its own -- its schedule tables and plans -- that shares the packed weights; the two most recent of those stay resident."""
        sampler = self.shape_sampler if sampler is None else sampler
        steps = self.ddim_steps if steps is None else int(steps)
        from ..samplers import ShapeDenoiser
        from ..schedules import SHAPE_SAMPLERS
        if sampler not in SHAPE_SAMPLERS:
            raise ValueError('shape_sampler must be one of %s, got %r' % (SHAPE_SAMPLERS, sampler))
        if steps < 1:
            raise ValueError('shape_steps must be a positive step count, got %r' % (steps,))
        if sampler == 'ddim' and steps == self.ddim_steps:
            if self._den is None or self._den.S != self._expected_steps() or self._den.ddim_eta != float(ddim_eta) \
                    or self._den.sampler != 'ddim':
                self._den = ShapeDenoiser(self.df, self.df_conf.model.params, ddim_steps=self.ddim_steps,
                                          device=_hip_device(_dev(self.df)), z_shape=self.z_shape, ddim_eta=ddim_eta)
            return self._den
        key = (sampler, steps, float(ddim_eta))
        den = self._dens.get(key)
        if den is None:
            w = self._den.w if self._den is not None else next((d.w for d in self._dens.values()), None)
            den = ShapeDenoiser(self.df, self.df_conf.model.params, ddim_steps=steps, device=_hip_device(_dev(self.df)),
                                z_shape=self.z_shape, ddim_eta=ddim_eta, sampler=sampler, weights=w)
            while len(self._dens) >= 2:
                self._dens.pop(next(iter(self._dens)))
            self._dens[key] = den
        return den

    def _expected_steps(self):
        return len(range(0, self.df_conf.model.params.timesteps,
                         self.df_conf.model.params.timesteps // self.ddim_steps))

    def _encoder(self):
        if getattr(self, '_enc', None) is None:
            from ..samplers import VQEncoder
            self._enc = VQEncoder(self.vqvae, _hip_device(_dev(self.vqvae)))
        return self._enc

    def keep_inputs(self, keep_nodes, keep_sdfs, n_objects, device):
        """``keep_nodes`` / ``keep_sdfs`` of the sampling calls -> (x0 [O,C,D,H,W], mask [O], rows, sdf rows [len(rows),1,64,64,64])
        of the masked DDIM loop: the kept SDFs go through ``VQVAE.encode_no_quant`` (samplers.VQEncoder)."""
        from ..samplers import keep_selection
        keep_nodes = [int(t) for t in (keep_nodes.tolist() if torch.is_tensor(keep_nodes) else keep_nodes)]
        sdfs = torch.as_tensor(keep_sdfs)
        if sdfs.dim() != 5 or sdfs.shape[0] != len(keep_nodes) or sdfs.shape[1] != 1:
            raise ValueError('keep_sdfs must be [len(keep_nodes), 1, D, H, W] (one truncated SDF per entry of keep_nodes); got %s '
                             'for %d nodes' % (tuple(sdfs.shape), len(keep_nodes)))
        mask, rows, src = keep_selection(keep_nodes, n_objects)
        x0 = torch.zeros((n_objects,) + tuple(self.z_shape), device=device)
        sel = sdfs[src].to(device).float().contiguous() if rows else sdfs[:0].to(device).float()
        if rows:
            x0[rows] = self._encoder().encode_no_quant(sel, sync=False)
        return x0, mask.to(device), rows, sel

    def check_complete(self, complete_nodes=None, complete_sdfs=None, complete_ranges=None, complete_masks=None, keep_nodes=None,
                       gen_shape=True):
        """The ``complete_*`` keywords of the sampling calls, validated on the host (no device work; every refusal is a ValueError):
        returns None without them, else (nodes, sdfs, ranges or None, masks or None) with one entry per entry of ``complete_nodes``."""
        given = [k for k, v in zip(_COMPLETE_OPTS, (complete_nodes, complete_sdfs, complete_ranges, complete_masks)) if v is not None]
        if not given:
            return None
        if complete_nodes is None or complete_sdfs is None:
            raise ValueError('complete_nodes and complete_sdfs go together (got %s)' % ', '.join(given))
        if not gen_shape:
            raise ValueError('complete_nodes / complete_sdfs complete SHAPES: they need gen_shape=True')
        if (complete_ranges is None) == (complete_masks is None):
            raise ValueError('shape completion needs exactly one of complete_ranges (xyz ranges) and complete_masks (latent masks); '
                             'got %s' % ('both' if complete_ranges is not None else 'neither'))
        as_list = lambda v: [int(t) for t in (v.tolist() if torch.is_tensor(v) else v)]
        nodes = as_list(complete_nodes)
        both = sorted(set(nodes) & set(as_list(keep_nodes) if keep_nodes is not None else ()))
        if both:
            raise ValueError('nodes %s are in keep_nodes and in complete_nodes: a shape is kept whole or completed, not both' % both)
        sdfs = torch.as_tensor(complete_sdfs)
        if sdfs.dim() != 5 or sdfs.shape[0] != len(nodes) or sdfs.shape[1] != 1:
            raise ValueError('complete_sdfs must be [len(complete_nodes), 1, D, H, W] (one truncated SDF per entry of complete_nodes); '
                             'got %s for %d nodes' % (tuple(sdfs.shape), len(nodes)))
        zd = tuple(int(d) for d in self.z_shape[1:])
        if complete_ranges is not None:
            from ..postprocess import range_bounds
            ranges = [complete_ranges] if isinstance(complete_ranges, dict) else list(complete_ranges)
            if len(ranges) != len(nodes):
                raise ValueError('complete_ranges must hold one xyz range per entry of complete_nodes; got %d for %d nodes'
                                 % (len(ranges), len(nodes)))
            range_bounds(ranges, zd[0])                              # (the form of every entry)
            return nodes, sdfs, ranges, None
        masks = torch.as_tensor(complete_masks)
        if tuple(masks.shape) != (len(nodes), 1) + zd:
            raise ValueError('complete_masks must be [len(complete_nodes), 1, %d, %d, %d] (latent space, one value for all channels); '
                             'got %s for %d nodes' % (zd + (tuple(masks.shape), len(nodes))))
        if not bool(((masks == 0) | (masks == 1)).all()):
            raise ValueError('complete_masks: 0 (generate) or 1 (keep) per latent voxel')
        return nodes, sdfs, None, masks

    def complete_inputs(self, checked, x0, mask, device):
        """The completed nodes into the inputs of the masked loop: ``checked`` from check_complete, ``x0`` [O, C, D, H, W] and the
        per-object ``mask`` [O] of the kept nodes (keep_inputs; zeros without any).  Returns (x0, the voxel mask [O, 1, D, H, W]): a kept
        node is an all-ones row, a completed node carries the encoding of its WHOLE SDF (shape_comp, sdfusion_model.py:411-418) and
        the latent mask of its range.  Duplicates and out-of-range entries as samplers.keep_selection."""
        from ..samplers import keep_selection
        from ..postprocess import latent_range_mask
        nodes, sdfs, ranges, masks = checked
        O, zd = x0.shape[0], tuple(int(d) for d in self.z_shape[1:])
        vm = mask.to(device).float().reshape(O, 1, 1, 1, 1).expand(O, 1, *zd).contiguous()
        _, rows, src = keep_selection(nodes, O)
        if rows:
            x0[rows] = self._encoder().encode_no_quant(sdfs[src].to(device).float().contiguous(), sync=False)
            if ranges is not None:
                vm[rows] = latent_range_mask([ranges[k] for k in src], zd, device)
            else:
                vm[rows] = masks[src].to(device).float()
        return x0, vm

    def _decoder(self):
        if self._dec is None:
            from ..samplers import VQDecoder
            self._dec = VQDecoder(self.vqvae, _hip_device(_dev(self.vqvae)))
        return self._dec

    @torch.no_grad()
    def rel2shape(self, data, ddim_eta=0.0, noise=None, sync=True, step_noise=None, *, shape_sampler=None, shape_steps=None):
        """echo2shape.py:484-525: one latent noise shared by all objects, 100-step DDIM (eta 0, no CFG),
        then VQ-VAE decode_no_quant -> SDF [O,1,64,64,64].  ``noise`` f32[1,C,D,H,W] replaces the
        reference's wall-clock seeded draw (``torch.manual_seed(int(time.time()))``, :502).
        ``shape_sampler`` ('ddim' | 'plms') / ``shape_steps`` (keyword-only; None: the attributes ``shape_sampler`` / ``ddim_steps``):
        the sampler of the shape loop and its step count -- 'plms' is the reference's PLMSSampler, S + 1 evaluations for S steps."""
        self.switch_eval()
        self.set_input(data)
        den = self._denoiser(ddim_eta, shape_sampler, shape_steps)             # ddim_eta != 0: sigma_t * randn per step and object (``step_noise`` f32[S,O,C,D,H,W] or drawn)
        if noise is None:
            g = torch.Generator(device=den.device).manual_seed(int(time.time()))
            noise = torch.randn((1,) + tuple(self.z_shape), device=den.device, generator=g)
        # 'concat': c_s is a constant fourth input channel (echo2shape.py:234-235, network.py:26-28); 'crossattn' + mp
        # ignores it (the GCN output overwrites the context, openai_model_3d.py:843-844)
        z = den.sample(self.uc_rel, self.triples, noise1=noise, step_noise=step_noise,
                       c=self.rel if (self.df.conditioning_key == 'concat' or
                                      not self.df.diffusion_net.messsage_passing) else None)
        self.gen_z = z                      # the latents handed to the VQ-VAE (echo2shape.py:521-522), kept like gen_df
        self.gen_df = self._decoder().decode_no_quant(z, sync=sync)
        return self.gen_df


class _SceneModel(nn.Module):
    """Common graph front-end of Sg2ScDiffModel / Sg2BoxDiffModel (EchoScene.py:14-113, EchoLayout.py:9-93)."""

    def __init__(self, vocab, diff_opt, diffusion_bs, embedding_dim, batch_size, gconv_pooling, gconv_num_layers,
                 mlp_normalization, separated, replace_latent, residual, use_angles, use_clip, with_shape):
        super().__init__()
        diff_opt = escfg.to_plain(diff_opt)
        g = embedding_dim
        self.replace_all_latent = replace_latent
        self.batch_size, self.embedding_dim, self.vocab = batch_size, g, vocab
        self.use_angles, self.clip = use_angles, use_clip
        add = 512 if use_clip else 0
        self.obj_classes_list = list(set(vocab['object_idx_to_name']))
        self.edge_list = list(set(vocab['pred_idx_to_name']))
        num_objs, num_preds = len(self.obj_classes_list), len(self.edge_list)
        self.obj_embeddings_ec = Emb(num_objs + 1, 2 * g)
        self.pred_embeddings_ec = Emb(num_preds, 2 * g)
        self.obj_embeddings_dc = Emb(num_objs + 1, 2 * g)
        self.pred_embeddings_man_dc = Emb(num_preds, 2 * g)
        self.out_dim_ini_encoder = 2 * g + add
        self.out_dim_manipulator = 2 * g + add
        kw = dict(hidden_dim=4 * g, pooling=gconv_pooling, mlp_normalization=mlp_normalization, residual=residual)
        self.gconv_net_ec = GraphTripleConvNet(2 * g + add, 2 * g + add, num_layers=gconv_num_layers,
                                               output_dim=self.out_dim_ini_encoder, **kw)
        self.gconv_net_manipulation = GraphTripleConvNet(self.out_dim_ini_encoder + g + 2 * g + add, 2 * g + add,
                                                         num_layers=min(gconv_num_layers, 5),
                                                         output_dim=self.out_dim_manipulator, **kw)
        self.diff_cfg = diff_opt
        self.diffusion_bs = diffusion_bs if diff_opt.hyper.batch_size is None else diff_opt.hyper.batch_size
        self.s_l_separated = separated
        if separated:   # present in checkpoints, never used by sampling
            rel = dict(num_layers=gconv_num_layers, output_dim=self.out_dim_manipulator, **kw)
            if with_shape:
                self.gconv_net_ec_rel_s = GraphTripleConvNet(self.out_dim_manipulator + 2 * g + add, 2 * g + add, **rel)
            self.gconv_net_ec_rel_l = GraphTripleConvNet(self.out_dim_manipulator + 2 * g + add, 2 * g + add, **rel)
        if with_shape:
            self.ShapeDiff = EchoToShape(diff_opt)
            layers = [2 * g + add, 960, 1280]
            if self.ShapeDiff.df.conditioning_key == 'concat':
                layers = [2 * g + add, 1280, 4096]
            self.rel_s_mlp = mlp(layers, mlp_normalization, final_nonlinearity=False)
        self.LayoutDiff = EchoToLayout(diff_opt)
        self.lr_init, self.lr_step, self.lr_evo = diff_opt.hyper.lr_init, diff_opt.hyper.lr_step, diff_opt.hyper.lr_evo
        self._setup_w = None

    # -- bookkeeping the caller touches (eval_3dfront.py:390, SGDiff.py:29,49-84) ---------------------
    def lr_lambda(self, counter):
        if counter < self.lr_step[0]:
            return 1.0
        if counter < self.lr_step[1]:
            return self.lr_evo[0] / self.lr_init
        if counter < self.lr_step[2]:
            return self.lr_evo[1] / self.lr_init
        return self.lr_evo[2] / self.lr_init

    def optimizer_ini(self):
        params = list(self.parameters())
        if hasattr(self, 'ShapeDiff'):
            params += self.ShapeDiff.trainable_params
        self.optimizerFULL = optim.AdamW(params, lr=1e-4)
        self.scheduler = optim.lr_scheduler.LambdaLR(self.optimizerFULL, lr_lambda=self.lr_lambda)
        self.optimizers = [self.optimizerFULL]

    def invalidate(self):
        """Drop packed device images (call after weights change)."""
        self._setup_w = None
        self.LayoutDiff.invalidate()
        if hasattr(self, 'ShapeDiff'):
            self.ShapeDiff.invalidate()

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.invalidate()
        return r

    def forward(self, *a, **k):
        raise NotImplementedError('training (forward / select_sdfs) is out of scope of this build')

    # -- setup GCNs (once per sample) -----------------------------------------------------------------
    def _setup(self, enc_objs, enc_triples, enc_text, enc_rel, dec_objs, dec_triples, dec_text, dec_rel,
               change_rows=(), added_rows=(), manip_pred_table='pred_embeddings_ec'):
        """init_encoder + manipulate (EchoScene.py:143-157,181-195) on the HIP rows path.
        Returns obj_embed_ (uc), latent_obj_vecs after splicing (c), device tensors."""
        from ..plan import Builder, GraphIndex, GCNWeights, View, emit_gcn
        dev = _hip_device(_dev(self))
        if self._setup_w is None:
            # packed GCN weights + the three embedding tables the glue reads; dropped by invalidate()
            from ..plan import own
            # (parameters that already live on the device are read in place: samplers.state_dict_for)
            here = lambda v: v.detach() if (v.is_cuda and v.device == dev) else v.detach().cpu()
            sd = {k: here(v) for k, v in nn.Module.state_dict(self).items()
                  if k.startswith(('gconv_net_ec.', 'gconv_net_manipulation.', 'obj_embeddings_ec.', 'pred_embeddings_ec.',
                                   'pred_embeddings_man_dc.'))}
            # (the embedding tables live on the device: the lookups below are device-side row gathers, the CLIP features are
            #  never copied to the host -- VERDICT r2 #9)
            pool = self.gconv_net_ec.gconvs[0].pooling          # 'avg' (every shipped args.json) or 'sum'
            self._setup_w = (GCNWeights(sd, 'gconv_net_ec', dev, pool), GCNWeights(sd, 'gconv_net_manipulation', dev, pool),
                             {k: own(sd[k + '.weight'], dev) for k in ('obj_embeddings_ec', 'pred_embeddings_ec',
                                                                             'pred_embeddings_man_dc')})
        w_ec, w_man, tabs = self._setup_w
        sd = {k + '.weight': v for k, v in tabs.items()}
        g = self.embedding_dim

        def embed(objs, triples, text, rel, ptab):
            p = triples[:, 1].to(dev).long()
            oe = sd['obj_embeddings_ec.weight'].index_select(0, objs.to(dev).long())
            pe = sd[ptab + '.weight'].index_select(0, p)
            if self.clip:
                oe = torch.cat([text.detach().to(dev).float(), oe], 1)
                pe = torch.cat([rel.detach().to(dev).float(), pe], 1)
            return oe.contiguous(), pe.contiguous()

        enc_oe, enc_pe = embed(enc_objs, enc_triples, enc_text, enc_rel, 'pred_embeddings_ec')
        dec_oe, dec_pe = embed(dec_objs, dec_triples, dec_text, dec_rel, manip_pred_table)
        Oe, Od = enc_oe.shape[0], dec_oe.shape[0]
        D = self.out_dim_ini_encoder
        b = Builder(dev)
        g_enc = GraphIndex(enc_triples, Oe, dev)
        latent = emit_gcn(b, w_ec, g_enc, View(b.dev(enc_oe)), enc_oe.shape[1], View(b.dev(enc_pe)), enc_pe.shape[1])
        plan = b.finish()
        plan.run()
        latent = latent.t                                           # [Oe, D] on device
        # append zero rows for added nodes (EchoScene.py:478-486) and the 64-d change slot (:428-435,:393-398)
        if len(added_rows):
            rows = [latent[i:i + 1] for i in range(Oe)]
            for ad in added_rows:
                rows.insert(ad, torch.zeros(1, D, device=dev))
            latent = torch.cat(rows, 0)
        # the reference walks the node index upwards and draws for every index that is IN the list (EchoScene.py:428-435):
        # ascending order, one draw per distinct node, out-of-range entries never match
        change = torch.zeros(Od, g)
        for i in sorted({int(r) for r in change_rows if 0 <= int(r) < Od}):
            change[i] = torch.from_numpy(np.random.normal(0, 1, g)).float()
        man_in = torch.cat([latent, change.to(dev), dec_oe], 1).contiguous()
        b2 = Builder(dev)
        g_dec = GraphIndex(dec_triples, Od, dev)
        latent_m = emit_gcn(b2, w_man, g_dec, View(b2.dev(man_in)), man_in.shape[1], View(b2.dev(dec_pe)),
                            dec_pe.shape[1])
        plan2 = b2.finish()
        plan2.run()
        torch.cuda.synchronize()
        return dec_oe, latent, latent_m.t

    def _box_keep(self, keep_box_nodes, keep_boxes, keep_box_noise, n_objects, device):
        """``keep_box_nodes`` / ``keep_boxes`` / ``keep_box_noise`` of the sampling calls -> keyword arguments of the masked layout loop
        (LayoutDenoiser.sample): x0 [O, 8] with the kept nodes' rows, mask [O].  ``keep_boxes`` f32 [K, 8] = sizes | translations |
        angles in the model's normalised space -- ``torch.cat`` of the rows these calls return -- one row per entry of
        ``keep_box_nodes`` (indices into the decoder-side node list; duplicates and out-of-range entries as samplers.keep_selection)."""
        if (keep_box_nodes is None) != (keep_boxes is None):
            raise ValueError('keep_box_nodes and keep_boxes go together')
        if keep_box_nodes is None:
            if keep_box_noise is not None:
                raise ValueError('keep_box_noise without keep_box_nodes / keep_boxes')
            return {}
        from ..samplers import keep_selection
        nodes = [int(t) for t in (keep_box_nodes.tolist() if torch.is_tensor(keep_box_nodes) else keep_box_nodes)]
        boxes = torch.as_tensor(keep_boxes)
        D = self.LayoutDiff.bbox_dim
        if boxes.dim() != 2 or tuple(boxes.shape) != (len(nodes), D):
            raise ValueError('keep_boxes must be [len(keep_box_nodes), %d] (sizes | translations | angles, normalised: one row per '
                             'entry of keep_box_nodes); got %s for %d nodes' % (D, tuple(boxes.shape), len(nodes)))
        mask, rows, src = keep_selection(nodes, n_objects)
        x0 = torch.zeros(n_objects, D, device=device)
        if rows:
            x0[rows] = boxes[src].to(device).float()
        return dict(x0=x0, mask=mask.to(device), keep_noise=keep_box_noise)

    def _layout(self, triples, obj_embed_, relation_cond, noise=None, *, keep_box_nodes=None, keep_boxes=None, keep_box_noise=None,
                layout_sampler=None, layout_steps=None, layout_eta=None):
        kw = self._box_keep(keep_box_nodes, keep_boxes, keep_box_noise, obj_embed_.shape[0], obj_embed_.device)
        kw.update(layout_sampler=layout_sampler, layout_steps=layout_steps, layout_eta=layout_eta)
        self.LayoutDiff.set_input({'preds': triples, 'box': None, 'uc_b': obj_embed_, 'c_b': relation_cond,
                                   'obj_id_to_scene': None})
        return self.LayoutDiff.generate_layout_sg(box_dim=self.diff_cfg.layout_branch.denoiser_kwargs.in_channels,
                                                  noise=noise, **kw)

    def _splice(self, latent, latent_m, rows, strict=False):
        """the manipulator's rows for the touched nodes ``rows``, the original ones for the others (EchoScene.py:440-448) -- or the
        manipulator's for all of them (``replace_all_latent``).  Entries outside the node list are ignored (``manipulated_nodes``) or,
        ``strict`` (added nodes), indexed as they are: an IndexError tells the caller about a wrong ``missing_nodes``"""
        if self.replace_all_latent:
            return latent_m
        latent = latent.clone()
        for t in sorted(rows):
            if strict or 0 <= int(t) < latent.shape[0]:
                latent[t] = latent_m[t]
        return latent

    @staticmethod
    def _keep_vector(n, rows, device=None):
        """1 for an untouched node, 0 for one of ``rows``: f32 [n, 1] on ``device`` (EchoScene.py, EchoLayout.py:342-348), or -- no
        device -- the plain list only EchoLayout's _with_additions variant returns"""
        hit = {int(t) for t in rows}
        flags = [0 if i in hit else 1 for i in range(n)]
        return flags if device is None else torch.tensor(flags, dtype=torch.float32, device=device).reshape(n, 1)


class Sg2ScDiffModel(_SceneModel):
    def __init__(self, vocab, diff_opt, diffusion_bs=8, embedding_dim=128, batch_size=32, gconv_pooling='avg',
                 gconv_num_layers=5, mlp_normalization='none', separated=False, replace_latent=False,
                 residual=False, use_angles=False, use_clip=True):
        super().__init__(vocab, diff_opt, diffusion_bs, embedding_dim, batch_size, gconv_pooling, gconv_num_layers,
                         mlp_normalization, separated, replace_latent, residual, use_angles, use_clip, True)
        self.sample_obj = self.diff_cfg.shape_branch.sampling
        self._rel_w = None

    def invalidate(self):
        super().invalidate()
        self._rel_w = None

    def _rel_s(self, feat):
        """rel_s_mlp + unsqueeze(1) (EchoScene.py:413-416) on the rows path."""
        from ..plan import Builder, PackedLinear, View, seg, fold_bn
        from .. import hip
        dev = feat.device
        if self._rel_w is None:
            sd = {k: v.detach().cpu() for k, v in self.rel_s_mlp.state_dict().items()}
            if '1.running_mean' in sd:
                W0, b0 = fold_bn(sd, '0', '1')
                last = '3'
            else:
                W0, b0 = sd['0.weight'], sd['0.bias']
                last = '2'
            self._rel_w = (PackedLinear(W0, b0, dev), PackedLinear(sd[last + '.weight'], sd[last + '.bias'], dev))
        l0, l1 = self._rel_w
        b = Builder(dev)
        O = feat.shape[0]
        h = View(b.buf(O, l0.N))
        b.linear([seg(View(feat.contiguous()))], l0, O, h, act=hip.ACT_RELU)
        o = View(b.buf(O, l1.N))
        b.linear([seg(h)], l1, O, o)
        b.keep.append(feat)
        b.finish().run()
        torch.cuda.synchronize()
        return o.t.unsqueeze(1)

    def _layout_and_shapes(self, gen_shape, dec_objs, dec_triples, obj_embed_, latent, layout_noise, shape_noise, *,
                           keep_nodes=None, keep_sdfs=None, keep_noise=None, keep_box_nodes=None, keep_boxes=None,
                           keep_box_noise=None, shape_sampler=None, shape_steps=None, layout_sampler=None, layout_steps=None,
                           layout_eta=None, complete_nodes=None, complete_sdfs=None, complete_ranges=None, complete_masks=None):
        """The two loops only share the setup (the reference runs them back to back, EchoScene.py:402-419).  Here they are
        ONE replayed hipGraph: each replay is a DDIM shape step with ten ancestral layout steps on a parallel branch
        (samplers.sample_layout_and_shape), then the VQ-VAE decode.

        ``keep_nodes`` / ``keep_sdfs`` (shape-preserving sampling): the listed nodes keep the SDFs the caller hands in -- their encoded
        latents follow the forward-noised trajectory of the masked DDIM loop (and take part in every step's message passing) while
        the other nodes are generated; the returned rows ``keep_nodes`` are the caller's SDFs themselves.

        ``keep_box_nodes`` / ``keep_boxes`` (box-preserving sampling, independent of the above; with or without gen_shape): the listed
        nodes keep the normalised boxes the caller hands in (_box_keep) -- the masked ancestral layout loop -- and the returned
        sizes / translations / angles rows of those nodes are the caller's numbers bit for bit.

        ``shape_sampler`` / ``shape_steps``: sampler ('ddim' | 'plms') and step count of the shape loop (None: ``ShapeDiff.shape_sampler`` /
        ``ShapeDiff.ddim_steps``); they combine freely with both keep families.  With ``gen_shape=False`` no shape loop runs and they
        are not looked at (unlike ``keep_nodes``, which names inputs that would be dropped, they only choose how a loop would run).

        ``layout_sampler`` / ``layout_steps`` / ``layout_eta``: sampler ('ddpm' | 'ddim'), step count and eta of the LAYOUT loop (None:
        the attributes of ``LayoutDiff``, i.e. the ancestral loop over every trained timestep); with or without gen_shape, and with
        both keep families and the shape keywords.  Each replay of the fused graph then carries n_iter_layout // n_iter_shape layout
        steps (samplers.sample_layout_and_shape).

        ``complete_nodes`` / ``complete_sdfs`` + ``complete_ranges`` or ``complete_masks`` (shape completion, the reference's shape_comp:
        diffusion_shape/sdfusion_model.py:400-446): the WHOLE given SDF of a listed node is encoded, the latent voxels inside its
        range (or with mask 1) follow the forward-noised trajectory of that encoding and the others are generated, the node taking
        part in every step's message passing; its returned row is the decode of the final latent -- the kept region is not pasted
        back (the reference pastes nothing).  The encoder's receptive field sees the part outside the range too: a caller with a
        truly partial scan fills it with the truncation value first (postprocess.partial_shape gives ``shape_part``).  Combines with
        ``keep_nodes`` in ONE plan of the voxel loop (a kept node is an all-ones mask row; its returned row stays the caller's SDF);
        ``keep_noise`` is the one table of q_sample's draws for both; a node cannot be in both lists."""
        lopts = dict(layout_sampler=layout_sampler, layout_steps=layout_steps, layout_eta=layout_eta)
        self.LayoutDiff.layout_options(**{k[len('layout_'):]: v for k, v in lopts.items()})
        if (keep_nodes is None) != (keep_sdfs is None):
            raise ValueError('keep_nodes and keep_sdfs go together')
        comp = self.ShapeDiff.check_complete(complete_nodes, complete_sdfs, complete_ranges, complete_masks, keep_nodes, gen_shape)
        if not gen_shape:
            if keep_nodes is not None:
                raise ValueError('keep_nodes / keep_sdfs keep SHAPES: they need gen_shape=True')
            return None, self._layout(dec_triples, obj_embed_, latent, layout_noise, keep_box_nodes=keep_box_nodes, keep_boxes=keep_boxes, keep_box_noise=keep_box_noise,
                                      **lopts)
        bk = self._box_keep(keep_box_nodes, keep_boxes, keep_box_noise, obj_embed_.shape[0], obj_embed_.device)
        from ..samplers import sample_layout_and_shape
        uc = self._rel_s(obj_embed_)
        c = self._rel_s(latent)
        L, S = self.LayoutDiff, self.ShapeDiff
        L.set_input({'preds': dec_triples, 'box': None, 'uc_b': obj_embed_, 'c_b': latent, 'obj_id_to_scene': None})
        S.switch_eval()
        S.set_input({'obj_cat': dec_objs, 'triples': dec_triples, 'c_s': c, 'uc_s': uc})
        sden = S._denoiser(0.0, shape_sampler, shape_steps)
        need_c = S.df.conditioning_key == 'concat' or not S.df.diffusion_net.messsage_passing
        if shape_noise is None:       # the reference seeds this draw from the wall clock (echo2shape.py:502)
            g = torch.Generator(device=sden.device).manual_seed(int(time.time()))
            shape_noise = torch.randn((1,) + tuple(S.z_shape), device=sden.device, generator=g)
        kw, rows, kept = dict(shape_sampler=sden.sampler), [], None      # (the sampler ``sden`` was chosen by)
        if keep_nodes is not None:
            x0, mask, rows, kept = S.keep_inputs(keep_nodes, keep_sdfs, uc.shape[0], sden.device)
            kw.update(x0=x0, mask=mask, keep_noise=keep_noise)
        if comp is not None:
            if keep_nodes is None:
                x0, mask = torch.zeros((uc.shape[0],) + tuple(S.z_shape), device=sden.device), torch.zeros(uc.shape[0])
            x0, vmask = S.complete_inputs(comp, x0, mask, sden.device)
            kw.update(x0=x0, mask=vmask, keep_noise=keep_noise)
        if bk:
            kw.update(box_x0=bk['x0'], box_mask=bk['mask'], box_keep_noise=bk['keep_noise'])
        x, z = sample_layout_and_shape(L._denoiser(layout_sampler, layout_steps, layout_eta), sden, obj_embed_, dec_triples, uc, c if need_c else None,
                                       layout_noise=layout_noise, shape_noise=shape_noise, **kw)
        boxes = L.split_boxes(x)
        S.gen_z = z
        if rows:
            # decode only the generated nodes; the kept rows are the caller's SDFs, bit for bit
            gen = [i for i in range(z.shape[0]) if i not in set(rows)]
            out = torch.empty((z.shape[0],) + tuple(kept.shape[1:]), device=z.device)
            if gen:
                dec = S._decoder().decode_no_quant(z[gen], sync=False)
                if tuple(dec.shape[1:]) != tuple(kept.shape[1:]):
                    raise ValueError('keep_sdfs are %s per object, the decoder emits %s' % (tuple(kept.shape[1:]), tuple(dec.shape[1:])))
                out[gen] = dec
            out[rows] = kept
            torch.cuda.synchronize()
            S.gen_df = out
        else:
            S.gen_df = S._decoder().decode_no_quant(z, sync=True)
        return S.gen_df, boxes

    @torch.no_grad()
    def sample(self, dec_objs, dec_triplets, dec_text_feat, dec_rel_feat, gen_shape=False, layout_noise=None,
               shape_noise=None, *, keep_nodes=None, keep_sdfs=None, keep_noise=None, keep_box_nodes=None,
               keep_boxes=None, keep_box_noise=None, shape_sampler=None, shape_steps=None, layout_sampler=None,
               layout_steps=None, layout_eta=None, complete_nodes=None, complete_sdfs=None, complete_ranges=None, complete_masks=None):
        """EchoScene.py:388-420.  ``keep_nodes`` / ``keep_sdfs``, ``keep_box_nodes`` / ``keep_boxes`` and ``complete_nodes`` / ``complete_sdfs`` /
        ``complete_ranges`` / ``complete_masks`` (keyword-only): see _layout_and_shapes."""
        oe, _, latent_m = self._setup(dec_objs, dec_triplets, dec_text_feat, dec_rel_feat,
                                      dec_objs, dec_triplets, dec_text_feat, dec_rel_feat)
        sdf, boxes = self._layout_and_shapes(gen_shape, dec_objs, dec_triplets, oe, latent_m, layout_noise, shape_noise,
                                             keep_nodes=keep_nodes, keep_sdfs=keep_sdfs, keep_noise=keep_noise, keep_box_nodes=keep_box_nodes, keep_boxes=keep_boxes, keep_box_noise=keep_box_noise,
                                             shape_sampler=shape_sampler, shape_steps=shape_steps,
                            layout_sampler=layout_sampler, layout_steps=layout_steps, layout_eta=layout_eta,
                            complete_nodes=complete_nodes, complete_sdfs=complete_sdfs, complete_ranges=complete_ranges, complete_masks=complete_masks)
        return {'shapes': sdf}, boxes

    def _edited(self, enc, dec, touched, added, gen_shape, layout_noise, shape_noise, change_rows=None, strict=False, **opts):
        """the two editing calls: ``touched`` nodes take the manipulator's latent rows and are 0 in the returned keep vector, ``added``
        rows are inserted as zeros, ``change_rows`` (default: ``touched``) get the change noise; ``opts``: the options, by keyword"""
        oe, latent, latent_m = self._setup(*enc, *dec, change_rows=touched if change_rows is None else change_rows, added_rows=added)
        sdf, boxes = self._layout_and_shapes(gen_shape, dec[0], dec[1], oe, self._splice(latent, latent_m, touched, strict),
                                             layout_noise, shape_noise, **opts)
        return self._keep_vector(len(boxes['translations']), touched, oe.device), {'shapes': sdf}, boxes

    @torch.no_grad()
    def sample_with_changes(self, enc_objs, enc_triples, enc_text_feat, enc_rel_feat, dec_objs, dec_triplets,
                            dec_text_feat, dec_rel_feat, manipulated_nodes, gen_shape=False, layout_noise=None,
                            shape_noise=None, *, keep_nodes=None, keep_sdfs=None, keep_noise=None, keep_box_nodes=None,
                            keep_boxes=None, keep_box_noise=None, shape_sampler=None, shape_steps=None, layout_sampler=None,
               layout_steps=None, layout_eta=None, complete_nodes=None, complete_sdfs=None, complete_ranges=None, complete_masks=None):
        """EchoScene.py:422-472.  ``keep_nodes`` / ``keep_sdfs`` (keyword-only): see _layout_and_shapes."""
        return self._edited((enc_objs, enc_triples, enc_text_feat, enc_rel_feat),
                            (dec_objs, dec_triplets, dec_text_feat, dec_rel_feat),
                            list(manipulated_nodes), [], gen_shape, layout_noise, shape_noise,
                            keep_nodes=keep_nodes, keep_sdfs=keep_sdfs, keep_noise=keep_noise, keep_box_nodes=keep_box_nodes, keep_boxes=keep_boxes, keep_box_noise=keep_box_noise,
                            shape_sampler=shape_sampler, shape_steps=shape_steps,
                            layout_sampler=layout_sampler, layout_steps=layout_steps, layout_eta=layout_eta,
                            complete_nodes=complete_nodes, complete_sdfs=complete_sdfs, complete_ranges=complete_ranges, complete_masks=complete_masks)

    @torch.no_grad()
    def sample_with_additions(self, enc_objs, enc_triples, enc_text_feat, enc_rel_feat, dec_objs, dec_triplets,
                              dec_text_feat, dec_rel_feat, missing_nodes, gen_shape=False, layout_noise=None,
                              shape_noise=None, *, keep_nodes=None, keep_sdfs=None, keep_noise=None, keep_box_nodes=None,
                              keep_boxes=None, keep_box_noise=None, shape_sampler=None, shape_steps=None, layout_sampler=None,
               layout_steps=None, layout_eta=None, complete_nodes=None, complete_sdfs=None, complete_ranges=None, complete_masks=None):
        """EchoScene.py:474-532: zero rows inserted at ``missing_nodes[i] + i``; note the reference draws the
        change noise for rows listed in ``missing_nodes`` (:489-494) but splices / masks ``nodes_added``."""
        added = [m + i for i, m in enumerate(missing_nodes)]
        return self._edited((enc_objs, enc_triples, enc_text_feat, enc_rel_feat),
                            (dec_objs, dec_triplets, dec_text_feat, dec_rel_feat),
                            added, added, gen_shape, layout_noise, shape_noise, change_rows=list(missing_nodes), strict=True,
                            keep_nodes=keep_nodes, keep_sdfs=keep_sdfs, keep_noise=keep_noise, keep_box_nodes=keep_box_nodes, keep_boxes=keep_boxes, keep_box_noise=keep_box_noise,
                            shape_sampler=shape_sampler, shape_steps=shape_steps,
                            layout_sampler=layout_sampler, layout_steps=layout_steps, layout_eta=layout_eta,
                            complete_nodes=complete_nodes, complete_sdfs=complete_sdfs, complete_ranges=complete_ranges, complete_masks=complete_masks)

    def state_dict(self, epoch=None, counter=None, **kw):
        """EchoScene.py:534-543 when called with (epoch, counter); plain nn.Module.state_dict otherwise."""
        sd = super().state_dict(**kw)
        if epoch is None and counter is None:
            return sd
        sd.update({'epoch': epoch, 'counter': counter, 'opt': self.optimizerFULL.state_dict(),
                   'vqvae': self.ShapeDiff.vqvae_module.state_dict(),
                   'shape_df': self.ShapeDiff.df_module.state_dict()})
        return sd


class Sg2BoxDiffModel(_SceneModel):
    def __init__(self, vocab, diff_opt, diffusion_bs=8, embedding_dim=128, batch_size=32, gconv_pooling='avg',
                 gconv_num_layers=5, mlp_normalization='none', separated=False, replace_latent=False,
                 residual=False, use_angles=False, use_clip=True):
        super().__init__(vocab, diff_opt, diffusion_bs, embedding_dim, batch_size, gconv_pooling, gconv_num_layers,
                         mlp_normalization, separated, replace_latent, residual, use_angles, use_clip, False)

    # EchoLayout's manipulator uses pred_embeddings_man_dc (EchoLayout.py:154), EchoScene pred_embeddings_ec
    @torch.no_grad()
    def sampleBoxes(self, dec_objs, dec_triplets, encoded_dec_text_feat, encoded_dec_rel_feat, layout_noise=None, *,
                    keep_box_nodes=None, keep_boxes=None, keep_box_noise=None, layout_sampler=None, layout_steps=None, layout_eta=None):
        """EchoLayout.py:291-307.  ``keep_box_nodes`` / ``keep_boxes`` (keyword-only): those nodes keep the given normalised boxes
        (_SceneModel._box_keep); also on the two editing calls.  ``layout_sampler`` / ``layout_steps`` / ``layout_eta`` (keyword-only):
        sampler, step count and eta of the layout loop (EchoToLayout.layout_options); also on the two editing calls."""
        self.LayoutDiff.layout_options(layout_sampler, layout_steps, layout_eta)
        oe, _, latent_m = self._setup(dec_objs, dec_triplets, encoded_dec_text_feat, encoded_dec_rel_feat,
                                      dec_objs, dec_triplets, encoded_dec_text_feat, encoded_dec_rel_feat,
                                      manip_pred_table='pred_embeddings_man_dc')
        return self._layout(dec_triplets, oe, latent_m, layout_noise, keep_box_nodes=keep_box_nodes, keep_boxes=keep_boxes, keep_box_noise=keep_box_noise,
                            layout_sampler=layout_sampler, layout_steps=layout_steps, layout_eta=layout_eta)

    def _edited(self, enc, dec, touched, added, layout_noise, keep_list=False, **box_opts):     # (keep_list: the additions call)
        """the two editing calls: the ``touched`` nodes get the change noise (sic for additions: nodes_added here, EchoLayout.py:367-372;
        EchoScene draws it for missing_nodes), take the manipulator's latent rows and are 0 in the returned keep vector"""
        self.LayoutDiff.layout_options(*(box_opts.get(k) for k in _LAYOUT_OPTS))
        oe, latent, latent_m = self._setup(*enc, *dec, change_rows=touched, added_rows=added, manip_pred_table='pred_embeddings_man_dc')
        boxes = self._layout(dec[1], oe, self._splice(latent, latent_m, touched, strict=keep_list), layout_noise, **box_opts)
        return self._keep_vector(len(boxes['translations']), touched, None if keep_list else oe.device), boxes

    @torch.no_grad()
    def sampleBoxes_with_changes(self, enc_objs, enc_triples, enc_text_feat, enc_rel_feat, dec_objs, dec_triples,
                                 dec_text_feat, dec_rel_feat, manipulated_nodes, layout_noise=None, *, keep_box_nodes=None,
                                 keep_boxes=None, keep_box_noise=None, layout_sampler=None, layout_steps=None, layout_eta=None):
        # keep: f32 [O,1] tensor on the model's device (EchoLayout.py:342-348); only the _with_additions variant returns a list
        return self._edited((enc_objs, enc_triples, enc_text_feat, enc_rel_feat), (dec_objs, dec_triples, dec_text_feat, dec_rel_feat),
                            list(manipulated_nodes), [], layout_noise, keep_box_nodes=keep_box_nodes, keep_boxes=keep_boxes, keep_box_noise=keep_box_noise,
                            layout_sampler=layout_sampler, layout_steps=layout_steps, layout_eta=layout_eta)

    @torch.no_grad()
    def sampleBoxes_with_additions(self, enc_objs, enc_triples, enc_text_feat, enc_rel_feat, dec_objs, dec_triples,
                                   dec_text_feat, dec_rel_feat, missing_nodes, layout_noise=None, *, keep_box_nodes=None,
                                   keep_boxes=None, keep_box_noise=None, layout_sampler=None, layout_steps=None, layout_eta=None):
        added = [m + i for i, m in enumerate(missing_nodes)]
        return self._edited((enc_objs, enc_triples, enc_text_feat, enc_rel_feat), (dec_objs, dec_triples, dec_text_feat, dec_rel_feat),
                            added, added, layout_noise, keep_list=True, keep_box_nodes=keep_box_nodes, keep_boxes=keep_boxes, keep_box_noise=keep_box_noise,
                            layout_sampler=layout_sampler, layout_steps=layout_steps, layout_eta=layout_eta)

    def state_dict(self, epoch=None, counter=None, **kw):
        sd = super().state_dict(**kw)
        if epoch is None and counter is None:
            return sd
        sd.update({'epoch': epoch, 'counter': counter, 'opt': self.optimizerFULL.state_dict()})
        return sd


class SGDiff(nn.Module):
    """model/SGDiff.py:6-129 -- the facade ``scripts/eval_3dfront.py`` constructs and calls."""

    def __init__(self, type, diff_opt, vocab, replace_latent=False, with_changes=True, residual=False,
                 gconv_pooling='avg', with_angles=False, clip=True, separated=False):
        super().__init__()
        assert type in ['echoscene', 'echolayout'], '{} is not included'.format(type)
        assert replace_latent is not None and with_changes is not None
        self.type_, self.vocab, self.with_angles, self.epoch, self.diff_opt = type, vocab, with_angles, 0, diff_opt
        cls = Sg2ScDiffModel if type == 'echoscene' else Sg2BoxDiffModel
        self.diff = cls(vocab, diff_opt, diffusion_bs=16, embedding_dim=64, mlp_normalization='batch',
                        separated=separated, gconv_num_layers=5, gconv_pooling=gconv_pooling, use_angles=with_angles,
                        replace_latent=replace_latent, residual=residual, use_clip=clip)
        self.diff.optimizer_ini()
        self.counter = 0

    def forward_mani(self, *a, **k):
        raise NotImplementedError('training (forward_mani) is out of scope of this build')

    def load_networks(self, exp, epoch, strict=True, restart_optim=False, load_shape_branch=True):
        """SGDiff.py:49-84: same checkpoint layout ('opt', 'vqvae', 'shape_df', 'epoch', 'counter' + module keys)."""
        ckpt = torch.load(os.path.join(exp, 'checkpoint', 'model{}.pth'.format(epoch)), map_location='cpu')
        opt_state = ckpt.pop('opt', None)
        if load_shape_branch and self.type_ == 'echoscene':
            if 'vqvae' in ckpt and 'shape_df' in ckpt:
                self.diff.ShapeDiff.vqvae.load_state_dict(ckpt.pop('vqvae'))
                self.diff.ShapeDiff.df.load_state_dict(ckpt.pop('shape_df'))
                self.diff.ShapeDiff.df_module = self.diff.ShapeDiff.df
                self.diff.ShapeDiff.vqvae_module = self.diff.ShapeDiff.vqvae
                self.diff.ShapeDiff.invalidate()
                print('[*] shape branch has successfully been restored from: %s'
                      % os.path.join(exp, 'checkpoint', 'model{}.pth'.format(epoch)))
            else:
                print('no vqvae or shape_df recorded. Assume it is only the layout branch')
        if 'epoch' in ckpt and 'counter' in ckpt:
            self.epoch, self.counter = ckpt.pop('epoch'), ckpt.pop('counter')
        else:
            print('no epoch or counter recorded.')
        ckpt.pop('vqvae', None)
        ckpt.pop('shape_df', None)
        self.diff.load_state_dict(ckpt, strict=strict)
        print('[*] GCN and layout branch has successfully been restored from: %s'
              % os.path.join(exp, 'checkpoint', 'model{}.pth'.format(epoch)))
        if not restart_optim:
            self.diff.optimizerFULL.load_state_dict(opt_state)
            self.diff.scheduler = optim.lr_scheduler.LambdaLR(self.diff.optimizerFULL, lr_lambda=self.diff.lr_lambda,
                                                              last_epoch=int(self.counter - 1))

    def cuda(self, device=None):
        r = super().cuda(device)
        if self.type_ == 'echoscene':         # the reference places the shape nets by cfg.hyper.device (echo2shape.py:77);
            dev = _dev(self)                  # keeping them on the same GPU as the rest is what that amounts to
            self.diff.ShapeDiff.df.to(dev)
            self.diff.ShapeDiff.vqvae.to(dev)
        self.diff.invalidate()
        return r

    def _no_keep_without_shapes(self, kw, gen_shape=True):
        if self.type_ == 'echolayout' and any(kw.get(k) is not None for k in ('keep_nodes', 'keep_sdfs', 'keep_noise')):
            raise ValueError("keep_nodes / keep_sdfs keep SHAPES; an 'echolayout' model has no shape branch")
        if self.type_ == 'echolayout' and any(kw.get(k) is not None for k in _COMPLETE_OPTS):
            raise ValueError("complete_nodes / complete_sdfs complete SHAPES; an 'echolayout' model has no shape branch")
        if self.type_ == 'echoscene':       # the completion keywords are checked before any device work, as the layout keywords below
            self.diff.ShapeDiff.check_complete(*(kw.get(k) for k in _COMPLETE_OPTS), keep_nodes=kw.get('keep_nodes'), gen_shape=gen_shape)
        if self.type_ == 'echolayout' and any(kw.get(k) is not None for k in ('shape_sampler', 'shape_steps')):
            raise ValueError("shape_sampler / shape_steps choose the sampler of the SHAPE loop; an 'echolayout' model has no shape branch")
        # the layout keywords are checked before any device work (an unknown sampler, layout_steps / layout_eta without 'ddim', ...)
        self.diff.LayoutDiff.layout_options(*(kw.get(k) for k in _LAYOUT_OPTS))

    @staticmethod
    def _box_kw(kw):
        return {k: kw.get(k) for k in _BOX_OPTS + _LAYOUT_OPTS}

    def sample_box_and_shape(self, dec_objs, dec_triplets, encoded_dec_text_feat, encoded_dec_rel_feat, gen_shape=False,
                             **noise):
        """``keep_nodes`` (indices into the decoder-side node list) + ``keep_sdfs`` f32 [K,1,64,64,64] (keyword-only, with
        gen_shape=True): those nodes keep the given truncated SDFs -- rows ``keep_nodes`` of the returned ``shapes`` are the caller's
        tensors bit for bit -- and the other nodes are generated in their context (masked DDIM).  Also on the two editing calls.
        ``keep_box_nodes`` + ``keep_boxes`` f32 [K, 8] (keyword-only; 'echoscene' with or without gen_shape, and 'echolayout'): those
        nodes keep the given boxes -- rows laid out sizes | translations | angles in the model's normalised space, i.e. ``torch.cat`` of
        the rows this call returns (postprocess.scale_box_params / preprocess_angle2sincos bring metric boxes there) -- while the other
        nodes are placed in their context (the masked ancestral loop); the returned rows of the kept nodes are the caller's numbers
        bit for bit.  ``keep_box_noise`` f32 [T, O, 8]: the forward-noising draws (None: drawn on the device).  Independent of
        ``keep_nodes`` / ``keep_sdfs``; also on the two editing calls.
        ``shape_sampler`` ('ddim' | 'plms') + ``shape_steps`` (keyword-only; None: ``diff.ShapeDiff.shape_sampler`` / ``.ddim_steps``, i.e.
        DDIM with 100 steps): sampler and step count of the shape loop.  'plms' is the reference's PLMSSampler (pseudo linear multistep,
        S + 1 denoiser evaluations for S steps; eta = 0 and at least two timesteps, else ValueError); it combines with both keep
        families.  Also on the two editing calls.  With ``gen_shape=False`` there is no shape loop and they have no effect.
        ``layout_sampler`` ('ddpm' | 'ddim') + ``layout_steps`` + ``layout_eta`` (keyword-only; both model types, with or without
        gen_shape; None: ``diff.LayoutDiff.layout_sampler`` / ``.layout_steps`` / ``.layout_eta``, i.e. the ancestral loop over every
        trained timestep): 'ddim' runs the reference's DDIMSampler on the layout denoiser over a strided schedule of ``layout_steps`` of
        the trained timesteps (eta 0: deterministic; eta scales the per-step noise), e.g. ``layout_steps=100`` -- a tenth of the
        launches of the layout loop.  ``layout_noise`` is then f32 [n_iter + 1, O, 8] and ``keep_box_noise`` f32 [n_iter, O, 8] over the
        schedule's iterations.  ``layout_steps`` / ``layout_eta`` with 'ddpm', or an unknown name, is a ValueError.  They combine with
        ``keep_box_nodes`` / ``keep_boxes`` and with the shape keywords; also on the two editing calls.
        ``complete_nodes`` + ``complete_sdfs`` f32 [K,1,64,64,64] + exactly one of ``complete_ranges`` (K dicts {'x': (a, b), 'y': ...,
        'z': ...} in [-1, 1], the xyz_dict of the reference's get_partial_shape) and ``complete_masks`` f32 [K,1,16,16,16] of zeros and
        ones in latent space (keyword-only, with gen_shape=True): shape completion, the reference's shape_comp -- the whole given SDF is
        encoded, the latent voxels inside the range keep following it and the rest of the shape is generated in the context of the
        scene; the returned row is the decode of the final latent (no paste-back).  The encoder sees the part outside the range too:
        a truly partial scan is filled with 0.2 there first (postprocess.partial_shape).  Combines with ``keep_nodes`` (one voxel plan,
        ``keep_noise`` the one table for both; a node in both lists is a ValueError), ``shape_sampler='plms'``, ``shape_steps``,
        ``keep_box_nodes`` and the layout keywords; also on the two editing calls."""
        self._no_keep_without_shapes(noise, gen_shape)
        if self.type_ == 'echolayout':
            return self.diff.sampleBoxes(dec_objs, dec_triplets, encoded_dec_text_feat, encoded_dec_rel_feat,
                                         layout_noise=noise.get('layout_noise'), **self._box_kw(noise))
        shape_dict, layout_dict = self.diff.sample(dec_objs, dec_triplets, encoded_dec_text_feat, encoded_dec_rel_feat,
                                                   gen_shape=gen_shape, **noise)
        return {**shape_dict, **layout_dict}

    def sample_boxes_and_shape_with_changes(self, enc_objs, enc_triples, encoded_enc_text_feat, encoded_enc_rel_feat,
                                            dec_objs, dec_triples, encoded_dec_text_feat, encoded_dec_rel_feat,
                                            manipulated_nodes, gen_shape=False, **noise):
        self._no_keep_without_shapes(noise, gen_shape)
        if self.type_ == 'echolayout':
            return self.diff.sampleBoxes_with_changes(enc_objs, enc_triples, encoded_enc_text_feat, encoded_enc_rel_feat,
                                                      dec_objs, dec_triples, encoded_dec_text_feat, encoded_dec_rel_feat,
                                                      manipulated_nodes, layout_noise=noise.get('layout_noise'), **self._box_kw(noise))
        keep, shape_dict, layout_dict = self.diff.sample_with_changes(
            enc_objs, enc_triples, encoded_enc_text_feat, encoded_enc_rel_feat, dec_objs, dec_triples,
            encoded_dec_text_feat, encoded_dec_rel_feat, manipulated_nodes, gen_shape=gen_shape, **noise)
        return keep, {**shape_dict, **layout_dict}

    def sample_boxes_and_shape_with_additions(self, enc_objs, enc_triples, encoded_enc_text_feat, encoded_enc_rel_feat,
                                              dec_objs, dec_triples, encoded_dec_text_feat, encoded_dec_rel_feat,
                                              missing_nodes, gen_shape=False, **noise):
        self._no_keep_without_shapes(noise, gen_shape)
        if self.type_ == 'echolayout':
            keep, layout_dict = self.diff.sampleBoxes_with_additions(
                enc_objs, enc_triples, encoded_enc_text_feat, encoded_enc_rel_feat, dec_objs, dec_triples,
                encoded_dec_text_feat, encoded_dec_rel_feat, missing_nodes, layout_noise=noise.get('layout_noise'), **self._box_kw(noise))
            return layout_dict                 # sic: the reference drops ``keep`` here (SGDiff.py:113-115)
        keep, shape_dict, layout_dict = self.diff.sample_with_additions(
            enc_objs, enc_triples, encoded_enc_text_feat, encoded_enc_rel_feat, dec_objs, dec_triples,
            encoded_dec_text_feat, encoded_dec_rel_feat, missing_nodes, gen_shape=gen_shape, **noise)
        return keep, {**shape_dict, **layout_dict}

    def save(self, exp, outf, epoch, counter=None):
        torch.save(self.diff.state_dict(epoch, counter), os.path.join(exp, outf, 'model{}.pth'.format(epoch)))
