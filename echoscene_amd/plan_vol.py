"""Plan compiler for the 3-D latent-SDF denoiser (reference UNet3DModel.forward,
model/networks/diffusion_shape/openai_model_3d.py:816-863, block semantics :294-314 and
attention.py:172-245, 335-351).

Per-object vectors (time MLP, conv-pool stem code, shape GCN, ResBlock time projections,
cross-attention-with-one-key vectors) run on the fp32 "rows" path; everything with a voxel
dimension runs on the "volume" path (channels-last, fp16 MFMA operands, fp32 accumulate and
fp32 residual stream).
"""
import ctypes as C
import math
import torch

from . import hip
from .hip import ConvArgs, GNArgs, LNArgs, AttnArgs, GegluArgs, ToClArgs, StemArgs, BlendArgs, BlendVoxArgs, ConvC1Args, Op


# Planner constants of the volume path (round 5: module constants, not environment switches -- they decide which products a plan
# holds and which tensors exist, i.e. the bits; tests / A-B tools set the attributes).
VOL_FOLD_FFO = True        # FeedForward output + proj_out as ONE K-concatenated product (round 4: -11 launches per step)
VOL_GN_F16 = True          # a ResBlock's conv1 -> GroupNorm -> conv2 intermediate written once, as f16, with the conv's row-group sums
VOL_GN_PART_FUSED = True     # a split-K conv's reduction kernel also forms the next GroupNorm's partial sums (same bits, one launch less)
VOL_GN_RG_ANY = False      # tests: ask every producing conv for the row-group sums, whatever route it takes


def _gn_rg():
    """the library's route option `gn_rg` (es_vol_set_option): GroupNorm statistics from the producing conv's row-group sums"""
    buf = C.create_string_buffer(512)
    hip.lib().es_vol_options(buf, 512)
    opts = dict(kv.split('=') for kv in buf.value.decode().strip(';').split(';'))
    return int(opts.get('gn_rg', '1')) != 0


def _deciding_problem(cv):
    """A copy of a conv's arguments as the run that DECIDES takes them.  A deterministic shard follows the whole problem (O_hint > O;
    round 6: the reference shard, O_hint < 0): where that run forms row-group sums every run must too (its own launch may take a
    route that cannot form them -- k_rowgroup_stats then leaves the same bits), or two runs would normalise with differently
    rounded statistics."""
    q = ConvArgs.from_buffer_copy(cv)
    if q.O_hint > q.O or q.O_hint < 0:
        q.O, q.O_hint = abs(q.O_hint), 0
    return q


class Produced:
    """What the plan knows about a tensor one of its convs wrote: the op's index, the tensor's rows and columns, and the sums a
    GroupNorm may take its statistics from -- ``kind`` 'rowgroup' (fp32 tensor, [2][rows / 64][cols] from the conv's epilogue) or
    'f16' (the same sums of an f16-only intermediate, formed before the rounding); None: not asked for (yet)."""

    def __init__(self, op, rows, cols, sums=None, kind=None):
        self.op, self.rows, self.cols, self.sums, self.kind = op, rows, cols, sums, kind


class VolEmitters:
    """Volume-path op emitters: the base class of plan.Builder, whose __init__ declares the state they use (hints and caches)."""

    @property
    def fp32x(self):
        """fp32 activations, split-operand f16 contractions (3 x the K)"""
        return self.precision == 'fp32x'

    @property
    def fp32(self):
        """the fp32-operand routes: every operand buffer of the plan is fp32.  Assigning it (single-kernel tests) sets the precision."""
        return self.precision in ('fp32', 'fp32x')

    @fp32.setter
    def fp32(self, on):
        self.precision = 'fp32' if on else 'fp16'

    @property
    def _rg_stats(self):
        """view of the registry for tests: data_ptr -> (producer op, row-group sums) of the tensors whose sums a GroupNorm took"""
        return {p: (self.ops[r.op], r.sums) for p, r in self._produced.items() if r.kind == 'rowgroup'}

    @property
    def _f16_stats(self):
        """view for tests: data_ptr -> sums of the f16-only intermediates; assigning a dict registers sums formed outside the plan"""
        return {p: r.sums for p, r in self._produced.items() if r.kind == 'f16'}

    @_f16_stats.setter
    def _f16_stats(self, sums):
        self._produced.update((p, Produced(None, 0, 0, s, 'f16')) for p, s in sums.items())

    def _push(self, kind, field, a):
        op = Op()
        op.kind, op.lane = kind, 0
        setattr(op.u, field, a)
        self.ops.append(op)
        return len(self.ops) - 1

    def _conv_args(self, a_t, pc, O, dims, mode, bias, rowvec, res, skip, ncdhw, out_ld, skip_bytes):
        """The ConvArgs fields every conv route fills the same way -- operand, weight, shape, the fused 1x1 skip phase, bias, row
        vector, residual, out_ld -- with the plan's keep list, weight bytes and flops.  The outputs, the split and the statistics
        are the caller's.  ``skip_bytes``: count the skip weight's bytes too."""
        D, H, W = dims
        a = ConvArgs()
        a.a, a.w = a_t.data_ptr(), pc.w.data_ptr()
        a.O, a.D, a.H, a.W = O, D, H, W
        a.Cin, a.N, a.taps, a.mode = pc.Cin, pc.N, pc.taps, mode
        if skip is not None:
            a.a2, a.w2, a.Cin2 = skip[0].data_ptr(), skip[1].w.data_ptr(), skip[1].Cin
            self.weight_bytes += skip[1].weight_bytes if skip_bytes else 0
            self.flops += 2 * O * D * H * W * skip[1].Cin * pc.N
        bt = pc.b if bias is None else bias
        a.bias = bt.data_ptr() if bt is not None else None
        if rowvec is not None:
            a.rowvec, a.rowvec_ld = rowvec.ptr, rowvec.ld
        a.res = res.data_ptr() if res is not None else None
        a.out_ld = -1 if ncdhw else (pc.N if out_ld is None else out_ld)
        self.keep += [pc, bt, skip]
        self.weight_bytes += pc.weight_bytes
        self.flops += 2 * O * D * H * W * pc.cin_true * pc.taps * pc.N
        return a

    def conv(self, a_f16, pc, O, dims, mode=hip.CONV_SAME, bias=None, rowvec=None, res=None, out_f32=None,
             out_f16=None, skip=None, ncdhw=False, splitk=None, epilogue=0, out_ld=None, w_fold=None):
        """dims = (D,H,W) of the OUTPUT grid. skip = (raw_f16 tensor, PackedConv) for the fused 1x1 skip.  ``w_fold``: the folded
        image of an ES_CONV_UP_HW conv (PackedConv.w_fold; es_conv_args.w2) -- known here, BEFORE the split-K workspace is offered:
        a launch that the library sends to the folded kernel when it is unsplit stays without a workspace."""
        assert w_fold is None or (skip is None and mode == hip.CONV_UP_HW)
        if self.fp32x and a_f16.dtype == torch.float32:
            # split-operand route: the fp32 operand(s) -> [hi | lo | hi] f16 images, then the ordinary f16 launch on 3 Cin channels; an
            # f16 operand copy of the output is the fp32 output itself, as on the fp32 route
            assert isinstance(pc, PackedConvX3) and not epilogue
            a3 = self.split3(a_f16, pc.cin_part)
            if skip is not None:
                skip = (self.split3(skip[0], skip[1].cin_part), skip[1])
            return self.conv(a3, pc, O, dims, mode=mode, bias=bias, rowvec=rowvec, res=res, out_f32=self._out32(out_f32, out_f16),
                             skip=skip, ncdhw=ncdhw, splitk=splitk, out_ld=out_ld)
        if self.fp32 and not self.fp32x:
            # fp32-operand validation route: the same launch on es_conv_f32 (fp32 activations / weights, exact-fp32 MFMA), unsplit and
            # without statistics.  (Its weight_bytes have never counted the skip weight, unlike the f16 route's: kept as recorded.)
            assert isinstance(pc, PackedConv32) and a_f16.dtype == torch.float32
            a = self._conv_args(a_f16, pc, O, dims, mode, bias, rowvec, res, skip, ncdhw, out_ld, skip_bytes=False)
            a.out_f32 = self._out32(out_f32, out_f16).data_ptr()
            return self._push(hip.OP_CONV_F32, 'conv', a)
        a = self._conv_args(a_f16, pc, O, dims, mode, bias, rowvec, res, skip, ncdhw, out_ld, skip_bytes=True)
        a.out_f32 = out_f32.data_ptr() if out_f32 is not None else None
        a.out_f16 = out_f16.data_ptr() if out_f16 is not None else None
        a.epilogue = epilogue
        a.O_hint = self.o_hint
        M = O * dims[0] * dims[1] * dims[2]
        # eligibility from the WHOLE (or reference) problem's row count (O_hint): a shard and the unsharded run must take the same
        # can_split decision, or the library picks S from the global tile count for one and S = 1 for the other
        Mh = (-a.O_hint if a.O_hint < 0 else max(a.O_hint, O)) * (M // O)
        folded = False
        if w_fold is not None:
            # the folded route takes unsplit launches only: ask the library what THIS launch does without a workspace (a, as filled so
            # far: workspace NULL, splitk 0).  Where it names the folded kernel the op stays that way -- 12 taps unsplit beat 27 taps
            # split (profiles/up_fold_notes.md); everywhere else the launch gets workspace and split as any other conv
            a.w2 = w_fold.data_ptr()
            self.keep.append(w_fold)
            name = C.create_string_buffer(32)
            if hip.lib().es_conv_kernel_of(C.byref(a), name, 32) < 0:
                raise RuntimeError('es_conv_kernel_of: ' + hip.lib().es_last_error().decode())
            folded = name.value == b'ws_256_up_fold'
        if not folded and not ncdhw and Mh * pc.N <= 8192 * 5376 and pc.N % 4 == 0 and not epilogue:
            self._offer_workspace(a, splitk, M * pc.N)
        idx = self._push(hip.OP_CONV, 'conv', a)
        if out_f32 is not None and not ncdhw and not epilogue and (out_ld is None or out_ld == pc.N):
            # a GroupNorm that reads this tensor later may ask the conv for its sums (_gn_source); a buffer that a LATER conv rewrites
            # gets a fresh record, so its sums come from that conv, never the stale ones of the first producer
            self._produced[out_f32.data_ptr()] = Produced(idx, M, pc.N)
        return idx

    @staticmethod
    def _out32(out_f32, out_f16):
        """the one output of an fp32-operand launch: a request for an f16 operand copy is served by the fp32 output itself (in these
        modes every "f16" buffer of the plan is an fp32 tensor)"""
        out = out_f32 if out_f32 is not None else out_f16
        assert out is not None and out.dtype == torch.float32 and (out_f32 is None or out_f16 is None)
        return out

    def _offer_workspace(self, a, splitk, slab):
        """split-K scratch shared by all convs of the plan (ops are stream-ordered): the slabs of the launch that splits widest"""
        a.splitk = -1 if splitk is None else splitk
        a.workspace = 1                                  # (any non-NULL value: es_conv_split_of only asks whether there is one)
        S = hip.lib().es_conv_split_of(C.byref(a))       # round 6: the library says how many slabs it will write
        if S < 0:
            raise RuntimeError('es_conv_split_of: ' + hip.lib().es_last_error().decode())
        need = max(S, splitk or 0, 1) * slab
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.buf(need, scratch=True)
            for op in self.ops:
                if op.kind == hip.OP_CONV and op.u.conv.workspace:
                    op.u.conv.workspace = self._ws.data_ptr()
        a.workspace = self._ws.data_ptr()

    def split3(self, x32, C):
        """f16 [rows, 3 C] split-operand image of the fp32 tensor x32 [rows, C] (es_split_f16x3), as one op of the plan"""
        rows = x32.numel() // C
        out = self.buf(rows, 3 * C, dtype=torch.float16, scratch=True)
        a = ToClArgs()
        a.x, a.O, a.C, a.V, a.Cpad, a.out, a.out_is_f32 = x32.data_ptr(), rows, C, 1, C, out.data_ptr(), 2
        self._push(hip.OP_TO_CL, 'tocl', a)
        return out

    def conv_gn_intermediate(self, a_f16, pc, O, dims, rowvec=None):
        """A conv whose output is read ONLY by a GroupNorm -- the conv1 -> GroupNorm -> conv2 intermediate of a ResBlock
        (openai_model_3d.py:294-314, vqvae_modules.py:67-126), never part of the residual stream.  It is written ONCE, as f16 (the
        operand precision the GroupNorm emits anyway), with the GroupNorm's statistics formed from the conv's fp32 values before the
        rounding (es_conv_args.gn_stats_out): 6 B per element less HBM traffic than fp32 out + fp32 in.
        Only where the launch forms those sums itself (es_conv_emits_gn_stats); a deterministic shard follows the decision of
        the WHOLE problem and, when its own route cannot form them, writes fp32 as well (the sums then come from a pass over it:
        same order, same bits; the GroupNorm still reads the f16 tensor).  Returns the tensor the GroupNorm is to read."""
        M, V = O * dims[0] * dims[1] * dims[2], dims[0] * dims[1] * dims[2]
        if self.fp32:
            h32 = self.buf(M, pc.N, scratch=True)
            self.conv(a_f16, pc, O, dims, rowvec=rowvec, out_f32=h32)
            return h32
        h16 = self.buf(M, pc.N, dtype=torch.float16, scratch=True)
        idx = self.conv(a_f16, pc, O, dims, rowvec=rowvec, out_f16=h16)
        cv = self.ops[idx].u.conv
        L = hip.lib()
        if V % 64 == 0 and _gn_rg() and VOL_GN_F16 and L.es_conv_emits_gn_stats(C.byref(_deciding_problem(cv))) == 1:
            st = self.buf(2 * (M // 64) * pc.N, scratch=True)
            cv.gn_stats_out = st.data_ptr()
            if L.es_conv_emits_gn_stats(C.byref(cv)) != 1:
                h32 = self.buf(M, pc.N, scratch=True)
                cv.out_f32 = h32.data_ptr()
            self._produced[h16.data_ptr()] = Produced(idx, M, pc.N, st, 'f16')
            return h16
        h32 = self.buf(M, pc.N, scratch=True)
        cv.out_f32, cv.out_f16 = h32.data_ptr(), None
        # the f16 tensor is not used on this route: release it (it was M x N x 2 bytes of HBM held for nothing)
        self.scratch.discard(h16.data_ptr())
        self.keep[:] = [t for t in self.keep if t is not h16]
        del h16
        self._produced[h32.data_ptr()] = Produced(idx, M, pc.N)
        return h32

    def _rowgroup_producer(self, x, Cx, M, V):
        """The record of the conv op of this plan that writes the fp32 tensor x and would form its row-group sums in its own epilogue
        (es_conv_emits_gn_stats), or None: x comes from elsewhere (stem output, another plan), the shapes do not allow it, or the
        conv takes a route behind which the sums would cost a pass over the output -- what the GroupNorm's statistics pass costs."""
        rec = self._produced.get(x.data_ptr())
        if not _gn_rg() or V % 64 or rec is None or rec.rows != M or rec.cols != Cx:
            return None
        op = self.ops[rec.op]
        if op.kind != hip.OP_CONV or op.u.conv.out_f32 != x.data_ptr():
            return None
        # (VOL_GN_RG_ANY, tests: ask whatever the route -- the sums then come from k_rowgroup_stats behind the conv)
        if not VOL_GN_RG_ANY and hip.lib().es_conv_emits_gn_stats(C.byref(_deciding_problem(op.u.conv))) != 1:
            return None
        return rec

    def _rowgroup_sums(self, rec, x):
        """Row-group sums [2][rows / 64][cols] of x, requested from its producer op (es_conv_args.gn_stats_out) the first time"""
        cv = self.ops[rec.op].u.conv
        if rec.sums is None:
            rec.sums, rec.kind = self.buf(2 * (rec.rows // 64) * rec.cols, scratch=True), 'rowgroup'
            cv.gn_stats_out = rec.sums.data_ptr()
        assert rec.kind == 'rowgroup' and cv.gn_stats_out == rec.sums.data_ptr() and cv.out_f32 == x.data_ptr()
        return rec.sums

    def _gn_source(self, a, xs, groups):
        """Where the GroupNorm ``a`` over the inputs ``xs`` = [(tensor, channels)] takes its statistics from -- decided here and
        nowhere else; ``a`` and the producing op are patched to match.  'f16': the sums of the f16-only intermediate
        (conv_gn_intermediate); 'rowgroup': the producing convs' epilogue sums (every input must have them); 'part': the per-tile
        partial sums a split-K conv's reduction leaves; 'pass': a pass over the inputs."""
        x1, C1 = xs[0]
        M = a.O * a.V
        if self.fp32:                               # fp32-operand validation route: always a pass over x
            return 'pass'
        if x1.dtype == torch.float16:
            assert len(xs) == 1 and not a.raw_f16 and self._produced[x1.data_ptr()].kind == 'f16'
            a.x1_is_f16, a.stats1 = 1, self._produced[x1.data_ptr()].sums.data_ptr()
            return 'f16'
        recs = [self._rowgroup_producer(x, Cx, M, a.V) for x, Cx in xs]
        if all(r is not None for r in recs):
            sums = [self._rowgroup_sums(r, x) for r, (x, _) in zip(recs, xs)]
            a.stats1, a.stats2 = sums[0].data_ptr(), (sums[1].data_ptr() if len(xs) > 1 else None)
            return 'rowgroup'
        rec = self._produced.get(x1.data_ptr())
        if len(xs) == 1 and VOL_GN_PART_FUSED and rec is not None and rec.rows == M and rec.cols == C1:
            # x1 written by a split-K conv of this plan: its reduction kernel leaves this GroupNorm's per-tile partial sums
            # (es_conv_args.gn_part_out; k_gn_partial's own order, the same bits) and the statistics launch is dropped
            op = self.ops[rec.op]
            cv = op.u.conv
            if op.kind == hip.OP_CONV and cv.out_f32 == x1.data_ptr() and not cv.gn_part_out and not cv.gn_stats_out:
                cv.gn_part_groups = groups
                if hip.lib().es_conv_emits_gn_part(C.byref(cv)) == 1:
                    pb = self.buf(a.O * ((a.V + 7) // 8) * groups * 2, scratch=True)
                    cv.gn_part_out = a.part_in = pb.data_ptr()
                    return 'part'
                cv.gn_part_groups = 0
        return 'pass'

    def gn_scratch(self, need):
        """the statistics scratch of ``need`` floats, ONE for all GroupNorms of the plan (same stream, in order)"""
        if self._gn_stats is None or self._gn_stats.numel() < need:
            self._gn_stats = self.buf(need, scratch=True)
        return self._gn_stats

    def groupnorm(self, x1, C1, x2, C2, O, V, gamma, beta, eps, silu, y_f16, raw_f16=None, groups=32):
        a = GNArgs()
        a.x1, a.C1 = x1.data_ptr(), C1
        a.x2, a.C2 = (x2.data_ptr(), C2) if x2 is not None else (None, 0)
        a.O, a.V, a.groups, a.eps = O, V, groups, eps
        a.gamma, a.beta, a.silu = gamma.data_ptr(), beta.data_ptr(), int(silu)
        # es_groupnorm_vol: partials at the smallest voxel tile (8) + final stats
        a.stats = self.gn_scratch(O * ((V + 7) // 8) * groups * 2 + O * groups * 2).data_ptr()
        a.y_f16 = y_f16.data_ptr()
        a.raw_f16 = raw_f16.data_ptr() if raw_f16 is not None else None
        a.O_hint = self.o_hint
        if self.fp32:                               # fp32 operand out
            assert y_f16.dtype == torch.float32 and (raw_f16 is None or raw_f16.dtype == torch.float32)
            a.y_is_f32 = 1
        self._gn_source(a, [(x1, C1)] + ([(x2, C2)] if x2 is not None else []), groups)
        self.keep += [gamma, beta]
        return self._push(hip.OP_GN, 'gn', a)

    def layernorm(self, x, M, Cc, gamma, beta, y_f16):
        a = LNArgs()
        a.x, a.M, a.C, a.eps = x.data_ptr(), M, Cc, 1e-5
        a.gamma, a.beta, a.y_f16 = gamma.data_ptr(), beta.data_ptr(), y_f16.data_ptr()
        a.y_is_f32 = 1 if y_f16.dtype == torch.float32 else 0
        self.keep += [gamma, beta]
        return self._push(hip.OP_LN, 'ln', a)

    def attention(self, qkv, B, Ntok, heads, dhead, out_f16):
        a = AttnArgs()
        a.qkv, a.B, a.Ntok, a.heads, a.dhead = qkv.data_ptr(), B, Ntok, heads, dhead
        a.scale = float(dhead) ** -0.5
        a.out_f16 = out_f16.data_ptr()
        self.flops += 4 * B * heads * Ntok * Ntok * dhead
        return self._push(hip.OP_ATTN_F32 if self.fp32 else hip.OP_ATTN, 'attn', a)

    def geglu(self, h_f32, M, C4, out_f16):
        a = GegluArgs()
        a.h_f32, a.M, a.C4, a.out_f16 = h_f32.data_ptr(), M, C4, out_f16.data_ptr()
        a.out_is_f32 = 1 if out_f16.dtype == torch.float32 else 0
        return self._push(hip.OP_GEGLU, 'geglu', a)

    def to_cl(self, x, O, Cc, V, Cpad, out):
        a = ToClArgs()
        a.x, a.O, a.C, a.V, a.Cpad, a.out = x.data_ptr(), O, Cc, V, Cpad, out.data_ptr()
        a.out_is_f32 = 1 if out.dtype == torch.float32 else 0
        return self._push(hip.OP_TO_CL, 'tocl', a)

    def conv_c1(self, x, w, bias, O, dims, out_f32):
        """Conv3d(1, N, 3, padding 1) of the fp32 volume x [O, D, H, W] -> channels-last fp32 [O*D*H*W, N] (es_conv_c1_f32: the VQ-VAE
        encoder's conv_in); w f32 [N, 27]"""
        a = ConvC1Args()
        a.x, a.w, a.bias = x.data_ptr(), w.data_ptr(), (bias.data_ptr() if bias is not None else None)
        a.out_f32, a.out_f16 = out_f32.data_ptr(), None
        a.O, (a.D, a.H, a.W), a.N = O, dims, w.shape[0]
        self.keep += [w, bias]
        self.weight_bytes += w.numel() * 4
        self.flops += 2 * O * dims[0] * dims[1] * dims[2] * 27 * w.shape[0]
        return self._push(hip.OP_CONV_C1, 'conv_c1', a)

    def blend(self, x, x0, mask, noise, tab, step):
        """masked-DDIM blend (es_ddim_blend) of the latents x [O, ...] with the forward-noised x0 of the objects whose mask is 1;
        noise [S, O * n], tab [S, 2] (ShapeSchedule.keep_tab)"""
        a = BlendArgs()
        a.x, a.x0, a.mask, a.noise = x.data_ptr(), x0.data_ptr(), mask.data_ptr(), noise.data_ptr()
        a.O, a.n = x.shape[0], x[0].numel()
        a.noise_stride = noise.shape[1]
        a.tab, a.step = tab.data_ptr(), step.data_ptr()
        self.keep += [x0, mask, noise, tab]
        return self._push(hip.OP_DDIM_BLEND, 'blend', a)

    def blend_vox(self, x, x0, mask, noise, tab, step):
        """masked-DDIM blend with a mask per latent voxel (es_ddim_blend_vox: shape completion) of the latents x [O, C, ...] with the
        forward-noised x0 where mask [O, V] is 1 (V = voxels of one channel; the C channels share it); noise [S, O * C * V], tab [S, 2]"""
        a = BlendVoxArgs()
        a.x, a.x0, a.mask, a.noise = x.data_ptr(), x0.data_ptr(), mask.data_ptr(), noise.data_ptr()
        a.O, a.C, a.V = x.shape[0], x.shape[1], x[0, 0].numel()
        assert tuple(mask.shape) == (a.O, a.V), (tuple(mask.shape), a.O, a.V)
        a.noise_stride = noise.shape[1]
        a.tab, a.step = tab.data_ptr(), step.data_ptr()
        self.keep += [x0, mask, noise, tab]
        return self._push(hip.OP_DDIM_BLEND_VOX, 'blend_vox', a)

    def plms(self, kind, x, eps, coef, step, ring, xsave, inc_step=True, push=True):
        """a PLMS sampler op (es_plms_update / es_plms_first_a / es_plms_first_b, ``kind`` = hip.OP_PLMS*): x [O, ...], eps a tensor or
        a (slab) View, coef the DDIM table [S, 4], ring [3, n] the last three eps, xsave [n] (first iteration only).  ``push=False``: the op is returned, not
        appended (the first-iteration ops go into a plan of their own)"""
        a = hip.PlmsArgs()
        if isinstance(eps, View):
            assert eps.ld == eps.width and eps.col == 0
            a.eps, a.eps_nslab, a.eps_slab_stride = eps.ptr, eps.nslab, eps.slab_stride
            self.keep.append(eps.t)
        else:
            a.eps = eps.data_ptr()
        a.x, a.n = x.data_ptr(), x.numel()
        a.coef, a.coef_stride = coef.data_ptr(), coef.shape[1]
        a.step, a.inc_step = step.data_ptr(), 1 if (inc_step and kind == hip.OP_PLMS) else 0
        assert ring.shape[0] == 3 and ring.shape[1] >= x.numel() and xsave.numel() == x.numel() and coef.shape[1] == 4
        a.ring, a.ring_stride, a.xsave = ring.data_ptr(), ring.shape[1], xsave.data_ptr()
        self.keep += [ring, xsave, coef]
        if not push:
            op = Op()
            op.kind, op.lane = kind, 0
            op.u.plms = a
            return op
        return self._push(kind, 'plms', a)

    def stem(self, x, w, scratch, out, O, cin=3, ostride=0):
        a = StemArgs()
        a.x = x.data_ptr()
        a.w0, a.b0, a.w1, a.b1 = [t.data_ptr() for t in w]
        a.scratch, a.out, a.O = scratch.data_ptr(), out.data_ptr(), O
        a.Cin, a.x_ostride = cin, ostride
        self.keep += list(w)
        return self._push(hip.OP_STEM, 'stem', a)


# (plan.Builder derives from VolEmitters, so plan imports this module in front of that class: only names plan defines earlier are taken
#  here; GCNWeights and emit_gcn, which follow Builder there, are imported where they are used)
from .plan import PackedLinear, View, seg, own, mm64       # noqa: E402


def up_fold_weights(W):
    """The four 3 x 2 x 2 weights of a 3x3x3 conv behind a nearest x(1, 2, 2) up-sampling, float64 [4, N, Cin, 3, 2, 2], class =
    2 ph + pw for output parity ph = h & 1, pw = w & 1.  After the up-sampling two of the three taps along H (and along W) read the same
    input voxel: class ph = 0 reads input rows hi - 1, hi with w[kh = -1] and w[0] + w[+1], ph = 1 reads hi, hi + 1 with
    w[-1] + w[0] and w[+1]; W folds the same way.  What es_pack_conv_up_fold_f16 sums (and rounds to f16 once)."""
    W = W.detach().double().cpu()
    assert W.dim() == 5 and tuple(W.shape[2:]) == (3, 3, 3)
    fold = [lambda t, ax: torch.stack([t.select(ax, 0), t.select(ax, 1) + t.select(ax, 2)], ax),
            lambda t, ax: torch.stack([t.select(ax, 0) + t.select(ax, 1), t.select(ax, 2)], ax)]
    return torch.stack([fold[pw](fold[ph](W, 3), 4) for ph in (0, 1) for pw in (0, 1)])


class PackedConv:
    """f16 [Npad][taps][Cin32] image of a conv / linear weight + fp32 bias on the device.  ``up_fold``: also the folded image of a
    3x3x3 weight for ES_CONV_UP_HW launches (``w_fold``; es_conv_args.w2, include/echoscene_hip.h)."""

    def __init__(self, W, b, device, geglu=False, up_fold=False):
        on_gpu = torch.device(device).type == 'cuda'
        W = W.detach().float().contiguous()
        W = W.to(device) if on_gpu else W.cpu()
        self.geglu = False
        if geglu and W.dim() == 2 and (W.shape[0] // 2) % 112 == 0 and b is not None:
            # GEGLU fused into the contraction epilogue (ES_EPI_GEGLU): every 16-row group of the packed weight = the value rows
            # of 8 outputs, then their 8 gate rows (value = first half of the projection, attention.py:39-46), so the value and
            # the gate of an output land in lanes i16 and i16 ^ 8 of one MFMA tile (echoscene_hip.h: es_conv_args.epilogue)
            C4 = W.shape[0] // 2
            idx = (torch.arange(C4).view(-1, 1, 8) + torch.tensor([0, C4]).view(1, 2, 1)).reshape(-1)
            W = W.index_select(0, idx.to(W.device)).contiguous()
            b = b.detach().float().cpu()[idx].contiguous()
            self.geglu = True
        self.N, cin = W.shape[0], W.shape[1]
        self.taps = 1 if W.dim() == 2 else int(W[0, 0].numel())
        if self.taps not in (1, 27):
            raise ValueError('conv kernel must be 1x1x1 or 3x3x3')
        self.Cin = (cin + 31) // 32 * 32
        L = hip.lib()
        if self.N <= 4 and self.taps == 27 and self.Cin <= 64:   # consumed by the small-N kernels (VQ-VAE conv_out)
            W = W.cpu()
            out = torch.empty(self.N * self.taps * self.Cin, dtype=torch.int16)
            hip.check(L.es_pack_conv_rows_f16(C.c_void_p(W.data_ptr()), self.N, cin, self.taps,
                                              C.c_void_p(out.data_ptr())), 'es_pack_conv_rows_f16')
        elif on_gpu:
            # the tiled image is formed on the GPU from the uploaded fp32 weight (es_pack_conv_f16_dev: bit-identical to the host loop,
            # which was 6 of the 9 s of a process's first scene call)
            with torch.cuda.device(device):
                out = torch.empty(L.es_pack_conv_f16_size(self.N, self.Cin, self.taps), dtype=torch.int16, device=device)
                hip.check(L.es_pack_conv_f16_dev(hip.ptr(W), self.N, cin, self.taps, hip.ptr(out), hip.current_stream()), 'es_pack_conv_f16_dev')
        else:
            n = L.es_pack_conv_f16_size(self.N, self.Cin, self.taps)
            out = torch.empty(n, dtype=torch.int16)
            hip.check(L.es_pack_conv_f16(C.c_void_p(W.data_ptr()), self.N, cin, self.taps, C.c_void_p(out.data_ptr())),
                      'es_pack_conv_f16')
        self.w = out.to(device)
        self.w_fold = None
        if up_fold and self.taps == 27 and not (self.N <= 4 and self.Cin <= 64):
            n = L.es_pack_conv_up_fold_f16_size(self.N, self.Cin)
            if on_gpu:
                with torch.cuda.device(device):
                    self.w_fold = torch.empty(n, dtype=torch.int16, device=device)
                    hip.check(L.es_pack_conv_up_fold_f16_dev(hip.ptr(W), self.N, cin, hip.ptr(self.w_fold), hip.current_stream()),
                              'es_pack_conv_up_fold_f16_dev')
            else:
                self.w_fold = torch.empty(n, dtype=torch.int16)
                hip.check(L.es_pack_conv_up_fold_f16(C.c_void_p(W.data_ptr()), self.N, cin, C.c_void_p(self.w_fold.data_ptr())),
                          'es_pack_conv_up_fold_f16')
        self.b = None if b is None else own(b, device)
        self.weight_bytes = self.N * cin * self.taps * 2
        self.cin_true = cin


class PackedConv32:
    """fp32 [N][taps][Cin16] image of a conv / linear weight (the fp32-operand validation route, csrc/es_vol32.hip).  A GEGLU projection
    keeps its value | gate row order (the fp32 route applies GEGLU with its own kernel)."""

    def __init__(self, W, b, device, geglu=False):
        W = W.detach().float().contiguous().cpu()
        self.geglu = False
        self.N, cin = W.shape[0], W.shape[1]
        self.taps = 1 if W.dim() == 2 else int(W[0, 0].numel())
        if self.taps not in (1, 27):
            raise ValueError('conv kernel must be 1x1x1 or 3x3x3')
        self.Cin = (cin + 15) // 16 * 16
        L = hip.lib()
        out = torch.empty(L.es_pack_conv_f32_size(self.N, cin, self.taps), dtype=torch.float32)
        hip.check(L.es_pack_conv_f32(C.c_void_p(W.data_ptr()), self.N, cin, self.taps, C.c_void_p(out.data_ptr())), 'es_pack_conv_f32')
        self.w, self.w_fold = out.to(device), None
        self.b = None if b is None else own(b, device)
        self.weight_bytes = self.N * cin * self.taps * 4
        self.cin_true = cin


class PackedConvX3(PackedConv):
    """Split-operand weight image (round 6, precision 'fp32x'): w = w_hi + w_lo in f16 (22 bits of the mantissa), packed as ONE f16
    image over 3 Cin channels [w_hi | w_hi | w_lo] -- against the activation image [a_hi | a_lo | a_hi] (es_split_f16x3) the ordinary
    f16 contraction accumulates a_hi w_hi + a_lo w_hi + a_hi w_lo in fp32.  ``cin_part``: channels of one part (Cin of the fp32
    operand, padded to 32); GEGLU is applied by its own kernel, as on the fp32 route."""

    def __init__(self, W, b, device, geglu=False):
        W = W.detach().float()
        cin = W.shape[1]
        cp = (cin + 31) // 32 * 32
        if cp != cin:
            pad = torch.zeros((W.shape[0], cp - cin) + tuple(W.shape[2:]), dtype=W.dtype, device=W.device)
            W = torch.cat([W, pad], 1)
        hi = W.half().float()
        lo = (W - hi).half().float()
        super().__init__(torch.cat([hi, hi, lo], 1), b, device, geglu=False)
        self.cin_part, self.cin_true = cp, cin
        self.weight_bytes = self.N * cin * self.taps * 6


def _transformer_weights(sd, name, device, PackedConv):
    """the weights of SpatialTransformer3D ``name`` with its one BasicTransformerBlock; ``PackedConv``: the weight class of the precision"""
    dv = lambda k: own(sd[k], device)
    PL = lambda w, b: PackedLinear(sd[w], sd[b] if b else None, device)
    PC = lambda w, b: PackedConv(sd[w], sd[b] if b else None, device)
    d = {}
    tb = name + '.transformer_blocks.0'
    d['gn'] = (dv(name + '.norm.weight'), dv(name + '.norm.bias'))
    d['proj_in'] = PackedConv(sd[name + '.proj_in.weight'].flatten(1), sd[name + '.proj_in.bias'], device)
    d['ln1'] = (dv(tb + '.norm1.weight'), dv(tb + '.norm1.bias'))
    d['ln3'] = (dv(tb + '.norm3.weight'), dv(tb + '.norm3.bias'))
    d['qkv'] = PackedConv(torch.cat([sd[tb + '.attn1.to_q.weight'], sd[tb + '.attn1.to_k.weight'],
                                     sd[tb + '.attn1.to_v.weight']], 0), None, device)
    d['o1'] = PC(tb + '.attn1.to_out.0.weight', tb + '.attn1.to_out.0.bias')
    d['o2'] = PL(tb + '.attn2.to_out.0.weight', tb + '.attn2.to_out.0.bias')     # rows path
    d['ff1'] = PackedConv(sd[tb + '.ff.net.0.proj.weight'], sd[tb + '.ff.net.0.proj.bias'], device, geglu=True)
    d['ff2'] = PC(tb + '.ff.net.2.weight', tb + '.ff.net.2.bias')
    d['proj_out'] = PackedConv(sd[name + '.proj_out.weight'].flatten(1), sd[name + '.proj_out.bias'], device)
    # FeedForward output + proj_out as ONE K-concatenated product (round 4): with t3 = ff2(gg) + t2 (attention.py:243-245)
    # and out = proj_out(t3) + x_in (:385-396),  out = (Wp W2) gg + Wp t2 + (Wp b2 + bp) + x_in -- the kernel's second
    # contraction phase (a2 / w2) carries the t2 term; the [M, C] tensor t3 and one HBM-bound launch per block disappear
    if VOL_FOLD_FFO:
        W2, b2 = sd[tb + '.ff.net.2.weight'].double(), sd[tb + '.ff.net.2.bias'].double()
        Wp, bp = sd[name + '.proj_out.weight'].flatten(1).double(), sd[name + '.proj_out.bias'].double()
        d['ffo'] = PackedConv(mm64(Wp, W2).float(), None, device)
        d['po'] = PackedConv(Wp.float(), None, device)
        d['ffo_bias'] = (mm64(Wp, b2) + bp).float().contiguous().to(device)
    return d


class UNet3DWeights:
    def __init__(self, sd, net, device, precision='fp16'):
        """sd: state_dict of the UNet3DModel holder ``net`` (keys without 'diffusion_net.').  ``precision='fp32'``: fp32 weight
        images for the fp32-operand validation route."""
        self.precision = precision
        PackedConv = globals()[{'fp32': 'PackedConv32', 'fp32x': 'PackedConvX3'}.get(precision, 'PackedConv')]
        self.device, self.mc, self.topo = device, net.model_channels, net.topo
        self.enable_t_emb, self.mp = net.enable_t_emb, net.messsage_passing
        self.heads = net.num_heads
        self.concat = bool(getattr(net, 'concat', False))
        dv = lambda k: own(sd[k], device)
        PL = lambda w, b: PackedLinear(sd[w], sd[b] if b else None, device)
        PC = lambda w, b: PackedConv(sd[w], sd[b] if b else None, device)
        self.te0 = PL('time_embed.0.weight', 'time_embed.0.bias')
        self.te2 = PL('time_embed.2.weight', 'time_embed.2.bias')
        self.shape_t = None
        if self.mp:
            self.stem = [dv('shape_embeddings.0.weight'), dv('shape_embeddings.0.bias'),
                         dv('shape_embeddings.2.weight'), dv('shape_embeddings.2.bias')]
            self.stem_lin = PL('shape_embeddings.5.weight', 'shape_embeddings.5.bias')
            self.shape_t = PL('shape_time_emb.weight', 'shape_time_emb.bias') if net.enable_t_emb else None
            self.pred_table = sd['pred_embeddings.weight'].detach().float().cpu()
            from .plan import GCNWeights
            self.gcn = GCNWeights(sd, 'shape_code_graph_cov', device)
        inp, mid, out = net.topo
        names = [(f'input_blocks.{i}.{j}', it) for i, blk in enumerate(inp) for j, it in enumerate(blk)]
        names += [(f'middle_block.{j}', it) for j, it in enumerate(mid)]
        names += [(f'output_blocks.{i}.{j}', it) for i, blk in enumerate(out) for j, it in enumerate(blk)]
        self.items, self.emb_slices, self.ca = {}, {}, {}
        emb_w, emb_b, ca_v, ca_b, off = [], [], [], [], 0
        for name, it in names:
            kind, d = it[0], {}
            if kind == 'conv_in':
                d['conv'] = PC(name + '.weight', name + '.bias')
            elif kind == 'res':
                d['gn1'] = (dv(name + '.in_layers.0.weight'), dv(name + '.in_layers.0.bias'))
                d['conv1'] = PC(name + '.in_layers.2.weight', name + '.in_layers.2.bias')
                d['gn2'] = (dv(name + '.out_layers.0.weight'), dv(name + '.out_layers.0.bias'))
                d['conv2'] = PC(name + '.out_layers.3.weight', name + '.out_layers.3.bias')
                if (name + '.skip_connection.weight') in sd:
                    d['skip'] = PackedConv(sd[name + '.skip_connection.weight'].flatten(1), None, device)
                    # both biases are added once in the fused epilogue
                    d['bias2'] = (sd[name + '.out_layers.3.bias'].float() +
                                  sd[name + '.skip_connection.bias'].float()).contiguous().to(device)
                emb_w.append(sd[name + '.emb_layers.1.weight'])
                emb_b.append(sd[name + '.emb_layers.1.bias'])
                self.emb_slices[name] = (off, it[2])
                off += it[2]
            elif kind == 'attn' and self.concat:
                # AttentionBlock (openai_model_3d.py:317-363).  QKVAttentionLegacy orders the qkv rows
                # [head][q|k|v][ch]; the attention kernel wants [q | k | v] with heads inside each: row permutation.
                Cc = it[1]
                ch = Cc // self.heads
                perm = torch.cat([torch.cat([torch.arange(h * 3 * ch + part * ch, h * 3 * ch + (part + 1) * ch)
                                             for h in range(self.heads)]) for part in range(3)])
                d['gn'] = (dv(name + '.norm.weight'), dv(name + '.norm.bias'))
                d['qkv'] = PackedConv(sd[name + '.qkv.weight'].flatten(1)[perm], sd[name + '.qkv.bias'][perm], device)
                d['proj_out'] = PackedConv(sd[name + '.proj_out.weight'].flatten(1), sd[name + '.proj_out.bias'], device)
            elif kind == 'attn':
                d, tb = _transformer_weights(sd, name, device, PackedConv), name + '.transformer_blocks.0'
                # cross-attention with one key: to_out2(to_v2(ctx)) folded into one matrix per block (fp64)
                self.ca[name] = (len(ca_v), it[1])
                ca_v.append(mm64(sd[tb + '.attn2.to_out.0.weight'], sd[tb + '.attn2.to_v.weight']).float())
                ca_b.append(sd[tb + '.attn2.to_out.0.bias'])
            elif kind == 'down':
                d['conv'] = PC(name + '.op.weight', name + '.op.bias')
            elif kind == 'up':
                if precision == 'fp16' and not self.concat:
                    # nearest x2 on H, W only: the launch may multiply 12 folded taps instead of 27 (emit_unet3d_step attaches the image)
                    d['conv'] = PackedConv(sd[name + '.conv.weight'], sd[name + '.conv.bias'], device, up_fold=True)
                else:
                    d['conv'] = PC(name + '.conv.weight', name + '.conv.bias')
            self.items[name] = d
        self.emb_all = PackedLinear(torch.cat(emb_w, 0), torch.cat(emb_b, 0), device)
        self.cav_all = None if self.concat else PackedLinear(torch.cat(ca_v, 0), torch.cat(ca_b, 0), device)
        self.out_gn = (dv('out.0.weight'), dv('out.0.bias'))
        self.out_conv = PC('out.2.weight', 'out.2.bias')
        self.in_ch, self.out_ch = net.in_channels, net.out_channels


class Vol:
    """Where the volume path of a plan stands: the fp32 activation ``h`` [O * V(dims), C] of the O local objects, the conv op that
    wrote it (``last_op``), its f16 copy where one was asked for (``h16``), and whether the side branch is still to be joined."""

    def __init__(self, b, O, dims):
        self.b, self.O, self.dims = b, O, tuple(dims)
        self.h, self.C, self.last_op, self.h16 = None, 0, None, None
        self.join_pending = False
        self.f16 = torch.float32 if b.fp32 else torch.float16       # dtype of every contraction OPERAND buffer of the plan

    @property
    def V(self):
        return math.prod(self.dims)

    @property
    def M(self):
        return self.O * self.V

    def act(self, C, dims=None):
        """an fp32 activation [O * V, C]; like every buffer here written by the step before it is read (not stored in model files)"""
        return self.b.buf(self.O * math.prod(dims or self.dims), C, scratch=True)

    def operand(self, C):
        """a contraction operand [O * V, C]"""
        return self.b.buf(self.M, C, dtype=self.f16, scratch=True)

    def wrote(self, op, h, C=None, dims=None):
        """the conv op ``op`` wrote the new activation ``h``"""
        self.last_op, self.h, self.h16 = op, h, None
        self.C = self.C if C is None else C
        self.dims = self.dims if dims is None else tuple(dims)

    def h_operand(self):
        """f16 copy of the current fp32 activation (for convs that read it un-normalised), asked of the op that wrote it"""
        if self.b.fp32:
            return self.h                          # the fp32 activation is the operand
        if self.h16 is None:
            self.h16 = self.operand(self.C)
            self.b.ops[self.last_op].u.conv.out_f16 = self.h16.data_ptr()
        return self.h16

    def join_side(self):
        if self.join_pending:
            jn = Op()
            jn.kind, jn.lane = hip.OP_JOIN, 2
            self.b.ops.append(jn)
            self.join_pending = False


def _res(st, r, cout, eps, groups=lambda C: 32, skip=None, rowvec=None):
    """ResBlock of the UNet (openai_model_3d.py:294-314; ``skip`` = (tensor, channels): the input is [h | skip], ``rowvec``: the time
    projection) and of the VQ-VAE (vqvae_modules.py:67-126): GroupNorm + SiLU, conv1 (+ rowvec), GroupNorm + SiLU, conv2 + the
    input -- or, where the channel count changes, + the 1x1 skip of the raw input as a second phase of conv2's launch."""
    b, O, dm, M, V = st.b, st.O, st.dims, st.M, st.V
    x1, C1 = st.h, st.C
    x2, C2 = skip if skip is not None else (None, 0)
    y1 = st.operand(C1 + C2)
    raw = st.operand(C1 + C2) if 'skip' in r else None
    b.groupnorm(x1, C1, x2, C2, O, V, r['gn1'][0], r['gn1'][1], eps, True, y1, raw, groups=groups(C1 + C2))
    h1 = b.conv_gn_intermediate(y1, r['conv1'], O, dm, rowvec=rowvec)
    y2 = st.operand(cout)
    b.groupnorm(h1, cout, None, 0, O, V, r['gn2'][0], r['gn2'][1], eps, True, y2, groups=groups(cout))
    o = st.act(cout)
    if 'skip' in r:
        st.wrote(b.conv(y2, r['conv2'], O, dm, bias=r['bias2'], skip=(raw, r['skip']), out_f32=o), o, C=cout)
    else:
        assert x2 is None
        st.wrote(b.conv(y2, r['conv2'], O, dm, res=x1, out_f32=o), o, C=cout)


def _self_attention(st, gn, qkv_w, proj_w, heads, eps, groups=32):
    """AttentionBlock of the 'concat' UNet (openai_model_3d.py:317-363) and AttnBlock of the VQ-VAE (vqvae_modules.py:128-176, one
    head): GroupNorm, q | k | v as one product, attention over all voxels of the object, output projection + the input"""
    b, O, dm, M, Cc = st.b, st.O, st.dims, st.M, st.C
    xin = st.h
    yn = st.operand(Cc)
    b.groupnorm(xin, Cc, None, 0, O, st.V, gn[0], gn[1], eps, False, yn, groups=groups)
    qkv = st.operand(3 * Cc)
    b.conv(yn, qkv_w, O, dm, out_f16=qkv)
    at = st.operand(Cc)
    b.attention(qkv, O, st.V, heads, Cc // heads, at)
    o = st.act(Cc)
    st.wrote(b.conv(at, proj_w, O, dm, res=xin, out_f32=o), o)


def _resample(st, pc, mode, nd, w_fold=None):
    """Downsample / Upsample: one conv on the grid ``nd`` that reads the un-normalised activation"""
    a16 = st.h_operand()
    o = st.act(st.C, nd)
    st.wrote(st.b.conv(a16, pc, st.O, nd, mode=mode, out_f32=o, w_fold=w_fold), o, dims=nd)


def _conv_in(st, w, pc, net_in):
    cpad = getattr(pc, 'cin_part', pc.Cin)
    xcl = st.operand(cpad)                         # (channels padded to the weight image's Cin: 32, fp32 route 16)
    st.b.to_cl(net_in, st.O, w.in_ch, st.V, cpad, xcl)
    o = st.act(w.mc)
    st.wrote(st.b.conv(xcl, pc, st.O, st.dims, out_f32=o), o, C=w.mc)


def _transformer(st, d, name, heads, cav):
    """SpatialTransformer3D with one BasicTransformerBlock (attention.py:172-245, 335-351); ``cav``: this block's cross-attention
    vectors, a View at the first local object's row"""
    st.join_side()                                 # the cross-attention vectors are read from here on
    b, O, dm, M, Cc = st.b, st.O, st.dims, st.M, st.C
    xin = st.h
    yn = st.operand(Cc)
    b.groupnorm(xin, Cc, None, 0, O, st.V, d['gn'][0], d['gn'][1], 1e-6, False, yn)
    t0 = st.act(Cc)
    b.conv(yn, d['proj_in'], O, dm, out_f32=t0)
    l1 = st.operand(Cc)
    b.layernorm(t0, M, Cc, d['ln1'][0], d['ln1'][1], l1)
    qkv = st.operand(3 * Cc)
    b.conv(l1, d['qkv'], O, dm, out_f16=qkv)
    at = st.operand(Cc)
    b.attention(qkv, O, st.V, heads, Cc // heads, at)
    # x = attn1(norm1(x)) + x ; x = attn2(norm2(x), ctx) + x  (one key: + per-object vector)
    t2 = st.act(Cc)
    t2h = st.operand(Cc) if ('ffo' in d and not b.fp32) else None      # operand copy of t2 for the folded ff2 + proj_out product
    b.conv(at, d['o1'], O, dm, rowvec=cav, res=t0, out_f32=t2, out_f16=t2h)
    l3 = st.operand(Cc)
    b.layernorm(t2, M, Cc, d['ln3'][0], d['ln3'][1], l3)
    gg = st.operand(4 * Cc)
    if d['ff1'].geglu:                             # GEGLU in the contraction epilogue: the [M, 8C] fp32 tensor never exists
        b.conv(l3, d['ff1'], O, dm, out_f16=gg, epilogue=hip.EPI_GEGLU, out_ld=4 * Cc)
    else:
        gl = st.act(8 * Cc)
        b.conv(l3, d['ff1'], O, dm, out_f32=gl)
        b.geglu(gl, M, 4 * Cc, gg)
    o = st.act(Cc)
    if 'ffo' in d:
        st.wrote(b.conv(gg, d['ffo'], O, dm, bias=d['ffo_bias'], skip=(t2 if b.fp32 else t2h, d['po']), res=xin, out_f32=o), o)
    else:
        t3 = st.operand(Cc)
        b.conv(gg, d['ff2'], O, dm, res=t2, out_f16=t3)
        st.wrote(b.conv(t3, d['proj_out'], O, dm, res=xin, out_f32=o), o)
    b.tags[name + '.transformer_blocks.0:in'] = View(t0)
    b.tags[name + '.transformer_blocks.0:attn2'] = View(t2)


def _down(st, pc, concat):
    D, H, W = st.dims
    _resample(st, pc, hip.CONV_DOWN_DHW if concat else hip.CONV_DOWN_HW, (D // 2 if concat else D, H // 2, W // 2))


def _up(st, pc, concat):
    D, H, W = st.dims
    b = st.b
    # the folded image rides in w2 (no up-sampling conv has a skip phase); the op, its taps and its plan signature stay as they are
    # and the library takes the folded route where the launch is eligible (conv_route: ws_256_up_fold) -- Builder.conv() withholds
    # the split-K workspace from exactly those launches.  Not under o_hint: the canonical / sharded arithmetic is the 27-tap one
    wf = pc.w_fold if (b.up_fold and not concat and not b.fp32 and not b.o_hint) else None
    _resample(st, pc, hip.CONV_UP_DHW if concat else hip.CONV_UP_HW, (D * 2 if concat else D, H * 2, W * 2), w_fold=wf)


def _run_block(st, w, r, prefix, blk, skip=None):
    """the items of one input / middle / output block of the topology; ``skip`` = (tensor, channels) of the matching input block"""
    for j, it in enumerate(blk):
        name, kind = f'{prefix}.{j}', it[0]
        d = w.items[name]
        if kind == 'conv_in':
            _conv_in(st, w, d['conv'], r.net_in)
        elif kind == 'res':
            assert st.C + (skip[1] if skip is not None else 0) == it[1], (name, st.C, skip and skip[1], it[1])
            _res(st, d, it[2], 1e-5, skip=skip, rowvec=View(r.emb_all, col=w.emb_slices[name][0], ld=0, width=it[2]))
            skip = None
        elif kind == 'attn' and w.concat:
            _self_attention(st, d['gn'], d['qkv'], d['proj_out'], w.heads, 1e-5)
        elif kind == 'attn':
            cav = r.cavo[name]
            _transformer(st, d, name, w.heads, View(cav.t, col=cav.col, ld=cav.ld, width=cav.width, row=r.row0))
        elif kind == 'down':
            _down(st, d['conv'], w.concat)
        elif kind == 'up':
            _up(st, d['conv'], w.concat)
        st.b.tags[name] = View(st.h)


class Step:
    """What emit_unet3d_step hands back; a field a variant does not have is None.  For the caller: ``objbuf`` [O, uc | code | t] the
    GCN input (its uc columns are refreshed per scene), ``split`` the op index of the echo exchange, ``codes_local`` / ``codes_all``
    its send block and receive buffer, ``code_cols`` (first column, width) of the code inside objbuf, ``xc`` the 'concat' staging
    tensor, ``cdev`` the conditioning of the variants without message passing, ``pred_rows`` the predicate embeddings per triple.
    For the volume path: ``emb_all`` the time projections' table row, ``cavo`` the cross-attention vectors by block, ``row0`` the
    first local row inside them, ``net_in`` the network's NCDHW input."""

    def __init__(self):
        self.objbuf = self.codes_local = self.codes_all = self.code_cols = self.xc = self.cdev = self.pred_rows = None
        self.split, self.row0 = 0, 0
        self.emb_all, self.cavo, self.net_in = None, {}, None


def _emit_echo(b, w, g, r, x, uc_dev, step, lo, hi, V0, c_dev, tables, gather_rows):
    """The echo chain of the message-passing variants: conv-pool stem code of the local objects -> exchange (sharded) -> node
    vectors [uc | code | t] -> shape GCN over the FULL graph.  Returns the GCN output, a View of all O rows."""
    from .plan import emit_gcn
    O, Ol, gdim = g.O, hi - lo, 64
    ucw = uc_dev.shape[1]
    Dobj = ucw + gdim + (gdim if w.enable_t_emb else 0)
    objbuf = r.objbuf = b.buf(O, Dobj)
    objbuf[:, :ucw].copy_(uc_dev)
    code512 = b.buf(Ol, 512)
    if w.concat:
        assert c_dev is not None and ucw == V0 and tuple(c_dev.shape) == (Ol, V0), 'concat: uc_s / c_s must be [O, D*H*W]'
        xc = r.xc = b.buf(Ol, 5, V0)
        xc[:, 3].copy_(c_dev)                      # constant over the loop: written once at plan build
        b.copy(xc.data_ptr(), x.data_ptr(), 3 * V0 * 4, rows=Ol, dst_pitch=5 * V0 * 4, src_pitch=3 * V0 * 4)
        b.stem(xc, w.stem, b.buf(Ol, 32 * 512), code512, Ol, cin=4, ostride=5 * V0)
    else:
        b.stem(x, w.stem, b.buf(Ol, 32 * 512), code512, Ol)
    if Ol == O and not b.force_exchange:
        b.linear([seg(View(code512))], w.stem_lin, Ol, View(objbuf, col=ucw, ld=Dobj, width=gdim))
    else:
        # sharded: this rank's codes go to the (zero-padded, equal-size) send block of the echo all-gather; the gathered
        # [world * block, 64] buffer is copied into the GCN input by the first op after the exchange -- no torch op and
        # no allocation between the two graph launches of a step
        r.codes_local = b.buf(max(Ol, b.shard_block or Ol), gdim, zero=True)
        b.linear([seg(View(code512))], w.stem_lin, Ol, View(r.codes_local))
        r.codes_all = b.buf(max(gather_rows or O, O), gdim, zero=True)
    r.split = len(b.ops)                           # <- all-gather point of the multi-GPU loop
    r.code_cols = (ucw, gdim)
    if r.codes_all is not None:
        b.copy(objbuf.data_ptr() + ucw * 4, r.codes_all.data_ptr(), gdim * 4, rows=O, dst_pitch=Dobj * 4, src_pitch=gdim * 4)
    if w.enable_t_emb:
        b.rowsel(tables['t_lin'], step, View(objbuf, col=ucw + gdim, ld=Dobj, width=gdim), rows=O)
    pred = r.pred_rows = b.dev(w.pred_table[torch.from_numpy(g.p_host)])     # refreshed in place for a new graph
    ctx = emit_gcn(b, w.gcn, g, View(objbuf), Dobj, View(pred), pred.shape[1])
    b.tags.update(ctx=ctx, code=View(objbuf, col=ucw, ld=Dobj, width=gdim))
    return ctx


def _emit_conditioning(b, w, r, x, ctx, c_dev, lo, Ol, V0, rows):
    """How the conditioning reaches the volume path (``rows``: the objects of the per-object row buffers -- every object of the
    graph, or without message passing the local ones).  'concat': as an input channel of the staging tensor xc -- the GCN output rows
    of the local objects (the fifth channel), or c_s itself without message passing (the fourth; no GCN).  'crossattn': as the
    cross-attention vectors of ALL transformer blocks, ONE product over the GCN output / over c_s."""
    if w.concat:
        if w.mp:
            assert ctx.width == V0
            b.copy(r.xc[:, 4].data_ptr(), ctx.ptr + lo * ctx.ld * 4, V0 * 4, rows=Ol, dst_pitch=5 * V0 * 4, src_pitch=ctx.ld * 4)
        else:
            assert tuple(c_dev.shape) == (Ol, V0), 'concat: c_s must be [O, D*H*W]'
            xc = r.xc = b.buf(Ol, 4, V0)
            xc[:, 3].copy_(c_dev)
            b.copy(xc.data_ptr(), x.data_ptr(), 3 * V0 * 4, rows=Ol, dst_pitch=4 * V0 * 4, src_pitch=3 * V0 * 4)
        return
    if not w.mp:
        ctx = View(b.dev(c_dev))
        r.cdev = ctx.t                             # refreshed by the caller for every sample
    cav = b.buf(rows, w.cav_all.N)
    b.linear([seg(ctx)], w.cav_all, rows, View(cav))
    coff = 0
    for name, (k, Cc) in w.ca.items():
        r.cavo[name] = View(cav, col=coff, ld=w.cav_all.N, width=Cc)
        coff += Cc


def _fork_side(b, r, side0, main_ops):
    """The ops from ``side0`` on, except ``main_ops``, become a parallel graph branch (lane 2) that the caller joins later"""
    for k in range(side0, len(b.ops)):
        if k not in main_ops:
            b.ops[k].lane = 2
    fk = Op()
    fk.kind, fk.lane = hip.OP_FORK, 2
    b.ops.insert(side0, fk)
    r.split += 1 if r.split > side0 else 0


def emit_unet3d_step(b, w, g, x, uc_dev, step, eps_out, tables, dims=(16, 16, 16), lo=0, hi=None, c_dev=None, gather_rows=None):
    """One UNet3DModel.forward: x f32 [Ol,3,D,H,W] (NCDHW) -> eps_out f32 [Ol,3,D,H,W].  ``tables``: time_tables (all objects
    share t: the time MLP and its projections are table rows selected by ``step``).  Returns a Step.

    'concat' family (``w.concat``; c_dev f32 [Ol, V] = this rank's rows of c_s): the network input is the 5-channel
    NCDHW staging tensor xc = [x_t (3) | c_s (1) | GCN output (1)] (diffusion_shape/network.py:26-28,
    openai_model_3d.py:841-842); its first four channels feed the conv-pool stem.

    Object sharding (multi-GPU): this rank owns objects [lo, hi) of the O-node graph; x / eps_out hold only
    those.  The per-object vector ops (GCN over the FULL graph, projections) are computed for all O
    rows on every rank -- they are ~0.1 % of the FLOPs -- while every voxel op runs on the local objects only.
    The one cross-rank dependency is the conv-pool stem code of the other ranks' objects (the "echo"): the ops
    up to ``Step.split`` produce this rank's codes, the caller all-gathers them into ``codes_all`` and runs the rest.

    No echo message passing (sdfusion-txt2shape.yaml / sdfusion-txt2shape_concat.yaml): objects are independent and c_s (c_dev,
    this rank's rows) is the one cross-attention key ('crossattn') or the fourth input channel ('concat').  The per-object row
    buffers hold the local objects only; nothing is exchanged between ranks."""
    assert b.precision == w.precision, 'the builder was made for precision %r, the weights are %r' % (b.precision, w.precision)
    hi = g.O if hi is None else hi
    Ol, V0 = hi - lo, math.prod(dims)
    r = Step()
    # ---- per-object (rows path) ----
    side0 = len(b.ops)                             # first op of the per-object (echo) chain, see 'side branch' below
    ctx = None
    if w.mp:
        ctx = _emit_echo(b, w, g, r, x, uc_dev, step, lo, hi, V0, c_dev, tables, gather_rows)
        r.row0 = lo                                # first local row inside the per-object row buffers
    else:
        assert c_dev is not None, 'shape denoiser without message passing needs the conditioning c_s'
    r.emb_all = b.buf(1, w.emb_all.N)              # all objects share t: one table row, broadcast (rowvec_ld = 0)
    b.rowsel(tables['emb_all'], step, View(r.emb_all))
    emb_op = len(b.ops) - 1
    _emit_conditioning(b, w, r, x, ctx, c_dev, lo, Ol, V0, g.O if w.mp else Ol)
    r.net_in = r.xc if w.concat else x
    # ---- side branch: the echo chain (conv-pool stem, 5-layer GCN, cross-attention vectors: ~45 dependent launches of a few
    # microseconds) feeds nothing before the FIRST transformer block, while conv_in and the first ResBlocks only need the
    # latent and the time-embedding table row.  In the single-GPU 'crossattn' plan it therefore runs as a parallel graph
    # branch (lane 2) and is joined right before the first SpatialTransformer3D -- ~0.4 ms off the critical path per step.
    # (not with ES_LANES=1: emit_gcn's own FORK/JOIN pairs would then be nested inside this branch and every inner JOIN would
    #  make the main stream wait for the whole echo chain)
    st = Vol(b, Ol, dims)                          # ---- volume path: local objects only ----
    if w.mp and not w.concat and Ol == g.O and not b.use_lanes and not b.force_exchange:
        _fork_side(b, r, side0, (emb_op,))         # (the table row of the time projections stays on the main branch)
        st.join_pending = True
    inp, mid, out = w.topo
    hs = []
    for i, blk in enumerate(inp):
        _run_block(st, w, r, f'input_blocks.{i}', blk)
        hs.append((st.h, st.C))
    _run_block(st, w, r, 'middle_block', mid)
    for i, blk in enumerate(out):
        _run_block(st, w, r, f'output_blocks.{i}', blk, skip=hs.pop())
    st.join_side()                                 # (a topology without transformer blocks: join before the step ends)
    yo = st.operand(st.C)
    b.groupnorm(st.h, st.C, None, 0, st.O, st.V, w.out_gn[0], w.out_gn[1], 1e-5, True, yo)
    b.conv(yo, w.out_conv, st.O, st.dims, out_f32=eps_out, ncdhw=True)
    return r


# ------------------------------------------------------------------------------------------------
# VQ-VAE decode epilogue: VQVAE.decode_no_quant (vqvae_networks/network.py:95-103) ->
# VectorQuantizer nearest-code lookup (quantizer.py:68-119) -> post_quant_conv -> Decoder3D.forward
# (vqvae_modules.py:376-409; ResnetBlock :67-126, AttnBlock :128-176, Upsample :24-39)
# ------------------------------------------------------------------------------------------------
def _vq_groups(C):
    return C // 4 if C <= 32 else (32 if C % 32 == 0 else 30)          # Normalize(), vqvae_modules.py:13-21


def _vq_res_weights(d, p, device):
    """ResnetBlock p of a VQ-VAE half (vqvae_modules.py:67-126; d: that half's state dict without its prefix)"""
    r = dict(gn1=(own(d[p + '.norm1.weight'], device), own(d[p + '.norm1.bias'], device)),
             conv1=PackedConv(d[p + '.conv1.weight'], d[p + '.conv1.bias'], device),
             gn2=(own(d[p + '.norm2.weight'], device), own(d[p + '.norm2.bias'], device)),
             conv2=PackedConv(d[p + '.conv2.weight'], d[p + '.conv2.bias'], device))
    r['cin'], r['cout'] = d[p + '.conv1.weight'].shape[1], d[p + '.conv1.weight'].shape[0]
    if (p + '.nin_shortcut.weight') in d:
        r['skip'] = PackedConv(d[p + '.nin_shortcut.weight'].flatten(1), None, device)
        r['bias2'] = (d[p + '.conv2.bias'].float() + d[p + '.nin_shortcut.bias'].float()).contiguous().to(device)
    return r


def _vq_attn_weights(d, p, device):
    """AttnBlock p (vqvae_modules.py:128-176): q | k | v as one product"""
    Cc = d[p + '.q.weight'].shape[0]
    return dict(
        C=Cc, gn=(own(d[p + '.norm.weight'], device), own(d[p + '.norm.bias'], device)),
        qkv=PackedConv(torch.cat([d[p + '.q.weight'].flatten(1), d[p + '.k.weight'].flatten(1),
                                  d[p + '.v.weight'].flatten(1)], 0),
                       torch.cat([d[p + '.q.bias'], d[p + '.k.bias'], d[p + '.v.bias']], 0), device),
        proj=PackedConv(d[p + '.proj_out.weight'].flatten(1), d[p + '.proj_out.bias'], device))


class VQWeights:
    def __init__(self, sd, device):
        dv = lambda k: own(sd[k], device)
        PC = lambda w, b: PackedConv(sd[w], sd[b] if b else None, device)
        E = sd['quantize.embedding.weight'].detach().double()
        Wp = sd['post_quant_conv.weight'].detach().double().flatten(1)          # [3,3]
        self.codebook = own(E, device)
        self.lut = (mm64(E, Wp.t()) + sd['post_quant_conv.bias'].double()).float().contiguous().to(device)
        self.n_embed = E.shape[0]
        if E.shape[1] != 3:
            raise NotImplementedError('embed_dim != 3')
        d = {k[len('decoder.'):]: v for k, v in sd.items() if k.startswith('decoder.')}
        self.conv_in = PackedConv(d['conv_in.weight'], d['conv_in.bias'], device)
        res = lambda p: _vq_res_weights(d, p, device)
        self.mid1, self.mid2 = res('mid.block_1'), res('mid.block_2')
        self.attn = _vq_attn_weights(d, 'mid.attn_1', device)
        n_lvl = 1 + max(int(k.split('.')[1]) for k in d if k.startswith('up.'))
        self.levels = []
        for lvl in reversed(range(n_lvl)):
            blocks, bi = [], 0
            while f'up.{lvl}.block.{bi}.norm1.weight' in d:
                blocks.append(res(f'up.{lvl}.block.{bi}'))
                bi += 1
            up = None
            if (f'up.{lvl}.upsample.conv.weight') in d:
                up = PackedConv(d[f'up.{lvl}.upsample.conv.weight'], d[f'up.{lvl}.upsample.conv.bias'], device)
            self.levels.append((blocks, up))
        self.out_gn = (own(d['norm_out.weight'], device), own(d['norm_out.bias'], device))
        self.conv_out = PackedConv(d['conv_out.weight'], d['conv_out.bias'], device)


def _vq_mid(st, w):
    """mid.block_1 -> mid.attn_1 -> mid.block_2 of either VQ-VAE half; Normalize() has eps 1e-6 (vqvae_modules.py:13-21)"""
    _res(st, w.mid1, w.mid1['cout'], 1e-6, _vq_groups)
    _self_attention(st, w.attn['gn'], w.attn['qkv'], w.attn['proj'], 1, 1e-6, _vq_groups(st.C))
    _res(st, w.mid2, w.mid2['cout'], 1e-6, _vq_groups)


def _vq_out(st, gn, pc, out):
    """norm_out -> GELU -> conv_out into the NCDHW tensor ``out``"""
    yo = st.operand(st.C)
    st.b.groupnorm(st.h, st.C, None, 0, st.O, st.V, gn[0], gn[1], 1e-6, 2, yo, groups=_vq_groups(st.C))
    st.b.conv(yo, pc, st.O, st.dims, out_f32=out, ncdhw=True)
    return st.dims


def emit_vq_decode(b, w, z, sdf_out, Oc, zdims=(16, 16, 16)):
    """z f32 [Oc,3,16,16,16] -> sdf_out f32 [Oc,1,64,64,64] (one chunk of objects)."""
    from .hip import VQArgs
    st = Vol(b, Oc, zdims)
    zq = st.operand(32)
    a = VQArgs()
    a.z, a.codebook, a.lut = z.data_ptr(), w.codebook.data_ptr(), w.lut.data_ptr()
    a.O, a.V, a.n_embed, a.Cpad = Oc, st.V, w.n_embed, 32
    a.idx_out = None
    a.out_f16 = zq.data_ptr()
    b._push(hip.OP_VQ, 'vq', a)
    b.keep.append(w)
    o = st.act(w.conv_in.N)
    st.wrote(b.conv(zq, w.conv_in, Oc, st.dims, out_f32=o), o, C=w.conv_in.N)
    _vq_mid(st, w)
    for blocks, up in w.levels:
        for r in blocks:
            _res(st, r, r['cout'], 1e-6, _vq_groups)
        if up is not None:
            _resample(st, up, hip.CONV_UP_DHW, tuple(2 * d for d in st.dims))
    return _vq_out(st, w.out_gn, w.conv_out, sdf_out)


# ------------------------------------------------------------------------------------------------
# VQ-VAE encoder: VQVAE.encode_no_quant (vqvae_networks/network.py:84-88) = Encoder3D.forward (vqvae_modules.py:258-289) ->
# quant_conv.  The way from an SDF a user HAS to the latent space the shape denoiser works in (shape-preserving sampling).
# ------------------------------------------------------------------------------------------------
def fold_quant_conv(sd):
    """quant_conv (1x1x1, z_channels -> embed_dim) folded into the encoder's conv_out in fp64, the way ``VQWeights.lut`` folds
    post_quant_conv: quant_conv(conv_out(h)) = (Wq Wo) * h + (Wq bo + bq).  Returns (W [embed_dim, C, 3, 3, 3], b [embed_dim]), fp64."""
    Wo, bo = sd['encoder.conv_out.weight'], sd['encoder.conv_out.bias']
    Wq, bq = sd['quant_conv.weight'].flatten(1), sd['quant_conv.bias']
    if Wo.shape[0] != Wq.shape[1]:
        raise NotImplementedError('double_z encoders (conv_out has %d channels, quant_conv reads %d) are not supported'
                                  % (Wo.shape[0], Wq.shape[1]))
    Wf = mm64(Wq, Wo.flatten(1)).reshape((Wq.shape[0],) + tuple(Wo.shape[1:]))
    bf = mm64(Wq, bo) + bq.detach().double().to(Wf.device)
    return Wf, bf


class VQEncWeights:
    """The encoder half of the 'vqvae' checkpoint entry (sd: state dict of model.vqvae.VQVAE) + quant_conv, packed for the volume path."""

    def __init__(self, sd, device):
        d = {k[len('encoder.'):]: v for k, v in sd.items() if k.startswith('encoder.')}
        if d['conv_in.weight'].shape[1] != 1:
            raise NotImplementedError('the encoder reads one-channel SDF volumes')
        self.conv_in_w = own(d['conv_in.weight'].flatten(1), device)               # [ch, 27] fp32: es_conv_c1_f32
        self.conv_in_b = own(d['conv_in.bias'], device)
        self.ch = self.conv_in_w.shape[0]
        n_lvl = 1 + max(int(k.split('.')[1]) for k in d if k.startswith('down.'))
        self.levels = []
        for lvl in range(n_lvl):
            if any(k.startswith('down.%d.attn.' % lvl) for k in d):
                raise NotImplementedError('attention inside the encoder levels (attn_resolutions) is not supported')
            blocks, bi = [], 0
            while f'down.{lvl}.block.{bi}.norm1.weight' in d:
                blocks.append(_vq_res_weights(d, f'down.{lvl}.block.{bi}', device))
                bi += 1
            down = None
            if f'down.{lvl}.downsample.conv.weight' in d:
                down = PackedConv(d[f'down.{lvl}.downsample.conv.weight'], d[f'down.{lvl}.downsample.conv.bias'], device)
            self.levels.append((blocks, down))
        self.mid1, self.mid2 = _vq_res_weights(d, 'mid.block_1', device), _vq_res_weights(d, 'mid.block_2', device)
        self.attn = _vq_attn_weights(d, 'mid.attn_1', device)
        self.out_gn = (own(d['norm_out.weight'], device), own(d['norm_out.bias'], device))
        Wf, bf = fold_quant_conv(sd)
        self.conv_out = PackedConv(Wf.float(), bf.float(), device)
        self.embed_dim = Wf.shape[0]
        self.n_down = len([1 for _, dn in self.levels if dn is not None])


def emit_vq_encode(b, w, sdf, z_out, Oc, dims=(64, 64, 64)):
    """sdf f32 [Oc,1,64,64,64] -> z_out f32 [Oc,3,16,16,16] (one chunk of objects).  ``b.tags`` names the activation after conv_in
    and after every Downsample (parity debugging)."""
    st = Vol(b, Oc, dims)
    b.keep.append(w)
    o = st.act(w.ch)
    b.conv_c1(sdf, w.conv_in_w, w.conv_in_b, Oc, st.dims, o)
    st.wrote(None, o, C=w.ch)
    b.tags['conv_in'] = View(o)
    for lvl, (blocks, down) in enumerate(w.levels):
        for r in blocks:
            _res(st, r, r['cout'], 1e-6, _vq_groups)
        if down is not None:                       # (the Downsample pads the far face only)
            _resample(st, down, hip.CONV_DOWN_DHW_P01, tuple(d // 2 for d in st.dims))
            b.tags['down.%d' % lvl] = View(st.h)
    _vq_mid(st, w)
    return _vq_out(st, w.out_gn, w.conv_out, z_out)                            # conv_out with quant_conv folded in
