"""What the conv matrices share (tests/test_hip_conv_matrix.py: the f16 MFMA kernels; tests/test_hip_conv32_matrix.py: k_conv_f32): the
operands of a case, its float64 reference with the error of the same computation in fp32 on the CPU, and the bookkeeping of the
guarded buffers (tests/guarded_buffers.py).  A plain module: no fixtures, no test."""
import numpy as np
import torch
import torch.nn.functional as F

import conv_matrix_cases as cm


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


def cl(x):          # NCDHW -> [O*V, C]
    return x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1]).contiguous()


def problem(case, f16_operands=True):
    """the operands (fp16-rounded where the kernels take f16; ``f16_operands=False``: unrounded fp32, for the fp32-operand kernel), the
    fp64 reference and e32, the error of the fp32 CPU computation"""
    O, (D, H, W), Cin, N, taps, mode = case['O'], case['dims'], case['Cin'], case['N'], case['taps'], case['mode']
    V = D * H * W
    op = (lambda t: t.half().float()) if f16_operands else (lambda t: t)
    p = dict(x=op(rnd((O, Cin) + cm.input_dims(mode, case['dims']), 1)),
             wt=op(rnd((N, Cin, 3, 3, 3) if taps == 27 else (N, Cin), 2) / np.sqrt(Cin * taps)), bias=rnd((N,), 3))
    if case['rowvec']:
        p['rowvec'] = rnd((O, N), 4)
    if case['res']:
        p['res'] = rnd((O * V, N), 5)
    if case['Cin2']:
        p['xs'] = op(rnd((O, case['Cin2'], D, H, W), 6))
        p['ws'] = op(rnd((N, case['Cin2']), 7) / np.sqrt(case['Cin2']))

    def compute(dt):
        x, wt = p['x'].to(dt), p['wt'].to(dt)
        if taps == 1:
            y = cl(x) @ wt.t()
        else:
            if mode == cm.SAME:
                y = F.conv3d(x, wt, padding=1)
            elif mode == cm.DOWN_HW:
                y = F.conv3d(x, wt, stride=(1, 2, 2), padding=1)
            elif mode == cm.DOWN_DHW:
                y = F.conv3d(x, wt, stride=2, padding=1)
            elif mode == cm.DOWN_DHW_P01:
                y = F.conv3d(F.pad(x, (0, 1, 0, 1, 0, 1)), wt, stride=2)
            else:
                y = F.conv3d(F.interpolate(x, (D, H, W), mode='nearest'), wt, padding=1)
            if case['Cin2']:
                y = y + F.conv3d(p['xs'].to(dt), p['ws'].to(dt)[:, :, None, None, None])
            y = cl(y)
        y = y + p['bias'].to(dt)
        if case['rowvec']:
            y = y + p['rowvec'].to(dt).repeat_interleave(V, 0)
        if case['res']:
            y = y + p['res'].to(dt)
        if case['geglu']:
            y = y[:, :N // 2] * F.gelu(y[:, N // 2:])
        if case['out'] == 'ncdhw':
            y = y.reshape(O, V, N).permute(0, 2, 1).reshape(O * N, V).contiguous()
        return y

    p['ref'] = compute(torch.float64)
    p['scale'] = p['ref'].abs().max().item()
    p['e32'] = (compute(torch.float32).double() - p['ref']).abs().max().item() / p['scale']
    return p


def stray_findings(tag, inputs, outputs):
    """stray writes and unwritten elements of one launch: ``inputs`` [(name, GuardedInput)], ``outputs`` [(name, GuardedOutput or
    None)] -> a list of findings (empty: every input and guard unchanged, every output element finite)"""
    bad = []
    for nm, g in inputs:
        if not g.unchanged():
            bad.append('%s: input %s (or its guards) was written' % (tag, nm))
    for nm, o in outputs:
        if o is None:
            continue
        if not o.guards_unchanged():
            bad.append('%s: the guard rows of %s were written' % (tag, nm))
        fin = torch.isfinite(o.view)
        if not bool(fin.all()):
            rws = (~fin).any(1).nonzero().flatten()
            cls = (~fin).any(0).nonzero().flatten()
            bad.append('%s: %s holds %d non-finite elements (never written, or computed from a guard): rows %d..%d (%d of them), '
                       'columns %d..%d (%d of them)' % (tag, nm, int((~fin).sum()), rws[0], rws[-1], len(rws), cls[0], cls[-1], len(cls)))
    return bad
