"""GPU: every instantiation of the self-attention kernels against fp64, with the kernel asserted (the cases: tests/side_matrix_cases.py,
whose routes tests/test_side_matrix_cpu.py checks without a GPU): the seven k_attention<DP, 4, NRT> of es_attention_f16 and
k_attention_f32m<64 / 96>, k_attention_f32<64 / 96> of es_attention_f32.

One test per (case, input family).  For every launch:
  * the route: es_attention_route_of on the REAL argument struct of the plan names the kernel, the rows per workgroup and the grid
    that the table expects, or the launch is not run and the test fails;
  * stray accesses (tests/guarded_buffers.py): qkv sits between NaN guards (a key, a channel or a query row read from outside
    poisons a stored row); the output is NaN-filled between patterned guard rows: every row is written (by exactly one workgroup
    of the remapped order -- a row left out stays NaN, a workgroup on the wrong rows leaves others out), nothing outside is;
  * the values: float64 softmax(q k^T scale) v on the operands as the kernel receives them (fp16-rounded qkv for es_attention_f16),
    PER ELEMENT:  f16: err <= 2^-11 |ref| + 2^-25 + 2^-11 sum_j p_ij |v_j| + s vmax  (the stored value's rounding; the
    probabilities enter the second product rounded to f16);  fp32: err <= s vmax;  vmax = max |v| over the keys and channels of the
    row's head.  s is measured: the largest (err - rounding terms) / vmax over the matrix on an MI355X is 0 for the f16 kernels -- no
    element of any case leaves the rounding terms, the largest err / rounding terms is 0.75 (1x1x520x68, peaked) -- and 4.4e-6 for
    the fp32 kernels (1x2x200x70, peaked: __expf on logits of +-40; 6.5e-7 on the normal family) (profiles/side_matrix_notes.md; -s
    prints every case's); the bar is 4 x that, rounded up to one digit: 0 and 2e-5, never above 1e-4.  A lost key, a key of the
    ragged tile that is not masked or a skipped rescale is off by 1e-2 and more;
  * exact equalities (torch.equal): a second run leaves the same bits; a batch of B equals B single launches.
Input families (side_matrix_cases.ATTN_FAMILIES; the property each is named after is asserted on the fp64 scores):
  normal          N(0, 1.5^2), as tests/test_hip_vol.py::test_attention;
  first_tile_max  one large key among the first 64: no row maximum moves after tile 0 -- the branch that skips the rescale of O;
  last_tile_max   scores grow along the keys: every row's maximum moves in every tile, the last (ragged) tile included;
  peaked          scaled logits spread over about +-40: most probabilities underflow in f16;
  equal_keys      all keys of a head equal: the output is the mean of V.
One token (the output is V, rounded) is a case of its own."""
import pytest
import torch

import side_matrix_cases as sm
from guarded_buffers import GuardedInput, GuardedOutput

pytestmark = pytest.mark.gpu

# 4 x the largest measured (err - rounding terms) / vmax, one significant digit, rounded up (the docstring); never above 1e-4
S_F16 = 0.0
S_F32 = 2e-5
assert S_F16 <= 1e-4 and S_F32 <= 1e-4

PAIRS = [(c, f) for c in sm.ATTN_CASES for f in c['families']]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def make_qkv(case, family):
    """[B, Ntok, 3, heads, dhead] fp32 (f16-representable for the f16 kernels)"""
    B, H, N, d = case['B'], case['heads'], case['Ntok'], case['dhead']
    g = torch.Generator().manual_seed(21)
    t = torch.randn((B, N, 3, H, d), generator=g, dtype=torch.float32)
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    v *= 1.5
    if family == 'normal':
        q *= 1.5
        k *= 1.5
    elif family == 'first_tile_max':
        q *= 0.5
        k *= 0.5
        q[..., 0] = 2.0
        k[:, min(5, N - 1), :, 0] = 16.0
    elif family == 'last_tile_max':
        q *= 0.5
        k *= 0.5
        q[..., 0] = 8.0
        k[..., 0] = (16.0 * torch.arange(1, N + 1) / N).view(1, N, 1)
        k[:, N - 1, :, 0] = 20.0
    elif family == 'peaked':
        q *= 3.6
        k *= 3.6
    elif family == 'equal_keys':
        q *= 1.5
        k[:] = k[:, :1] * 1.5
    else:
        raise ValueError(family)
    if not case['fp32']:
        t = t.half().float()
    return t.contiguous()


def reference(case, t, dev):
    """float64 on the device: ref [B * Ntok, C], sum_j p |v| (same shape), vmax per element, the scaled scores [B, H, N, N]"""
    B, H, N, d = case['B'], case['heads'], case['Ntok'], case['dhead']
    td = t.to(dev).double()
    q, k, v = (td[:, :, i].permute(0, 2, 1, 3) for i in range(3))            # [B, H, N, d]
    s = q @ k.transpose(-1, -2) * float(torch.tensor(float(d) ** -0.5, dtype=torch.float32))
    p = torch.softmax(s, -1)
    f = lambda x: x.permute(0, 2, 1, 3).reshape(B * N, H * d)
    vmax = v.abs().amax(dim=(2, 3), keepdim=True).expand(B, H, N, d)
    return f(p @ v), f(p @ v.abs()), f(vmax), s


def check_family(case, family, s):
    N = case['Ntok']
    tiles = [s[..., k0:k0 + 64].amax(-1) for k0 in range(0, N, 64)]
    if family == 'first_tile_max':
        assert all(bool((tiles[0] > t).all()) for t in tiles[1:]), 'some row maximum lies behind the first key tile'
    if family == 'last_tile_max':
        run = tiles[0]
        for t in tiles[1:]:
            assert bool((t > run).all()), 'some row maximum does not move in some tile'
            run = t
    if family == 'peaked':
        assert (s.amax() - s.amin()).item() > 60 and bool(((s - s.amax(-1, keepdim=True)) < -17).float().mean() > 0.5)
    if family == 'equal_keys':
        assert bool((s.amax(-1) - s.amin(-1)).abs().max() < 1e-9)


class Launch:
    def __init__(self, dev, case, t, B=None):
        from echoscene_amd import hip
        from echoscene_amd.plan import Builder
        import echoscene_amd.plan_vol  # noqa: F401
        B = case['B'] if B is None else B
        H, N, d = case['heads'], case['Ntok'], case['dhead']
        dt = torch.float32 if case['fp32'] else torch.float16
        self.qkv = GuardedInput(dev, t.reshape(B * N, 3 * H * d), dt, N * 3 * H * d)
        self.out = GuardedOutput(dev, B * N, H * d, dt)
        b = Builder(dev)
        b.fp32 = case['fp32']
        i = b.attention(self.qkv.view, B, N, H, d, self.out.view)
        assert b.ops[i].kind == (hip.OP_ATTN_F32 if case['fp32'] else hip.OP_ATTN)
        self.route = sm.attn_route_of(hip.lib(), b.ops[i].u.attn, case['fp32'])
        self.builder = b

    def run(self):
        self.plan = self.builder.finish()
        self.plan.run()
        torch.cuda.synchronize()

    def findings(self, tag):
        bad = []
        if not self.qkv.unchanged():
            bad.append('%s: qkv (or its guards) was written' % tag)
        if not self.out.guards_unchanged():
            bad.append('%s: the guard rows of the output were written' % tag)
        nf = ~torch.isfinite(self.out.view)
        if bool(nf.any()):
            rws = nf.any(1).nonzero().flatten()
            bad.append('%s: the output holds %d non-finite elements (never written, or computed from a guard): rows %d..%d (%d of them)'
                       % (tag, int(nf.sum()), rws[0], rws[-1], len(rws)))
        return bad


@pytest.mark.parametrize('case,family', PAIRS, ids=['%s-%s' % (c['name'], f) for c, f in PAIRS])
def test_attention_matrix(dev, case, family):
    t = make_qkv(case, family)
    ref, pv_abs, vmax, scores = reference(case, t, dev)
    check_family(case, family, scores)
    del scores
    ln = Launch(dev, case, t)
    want = {k: case[k] for k in ('kernel', 'DP', 'rows', 'grid')}
    assert ln.route is not None and {k: ln.route[k] for k in want} == want, \
        '%s: routed to %s; the table says %s (not run)' % (case['name'], ln.route, want)
    ln.run()
    tag = '%s [%s] %s' % (case['name'], family, case['kernel'])
    bad = ln.findings(tag)
    out = ln.out.view.clone()
    err = torch.nan_to_num((out.double() - ref).abs(), nan=float('inf'))
    rounding = 0.0 if case['fp32'] else ref.abs() * 2.0 ** -11 + 2.0 ** -25 + pv_abs * 2.0 ** -11
    s = S_F32 if case['fp32'] else S_F16
    print('%s: largest (err - rounding) / vmax = %.3e (bar s = %.0e); largest err / (rounding + s vmax) = %.3f'
          % (tag, ((err - rounding).clamp(min=0) / vmax).max().item(), s, (err / (rounding + s * vmax)).max().item()))
    over = err - (rounding + s * vmax)
    if not bool((over <= 0).all()):
        wr, wc = divmod(int(over.argmax()), ref.shape[1])
        bad.append('%s: %d elements beyond the bound, worst at row %d (batch %d, token %d) channel %d (head %d): got %.6g, fp64 %.6g'
                   % (tag, int((over > 0).sum()), wr, wr // case['Ntok'], wr % case['Ntok'], wc, wc // case['dhead'], out[wr, wc].item(),
                      ref[wr, wc].item()))
    if case['Ntok'] == 1:                       # one token: the output is V, rounded
        v = t[:, :, 2].reshape(case['B'], -1).to(dev)
        if not torch.equal(out.float(), v.to(out.dtype).float()):
            bad.append('%s: the output of a one-token sequence is not V' % tag)
    # ---- exact equalities
    ln.out.refill()
    ln.plan.run()
    torch.cuda.synchronize()
    if not torch.equal(ln.out.view.view(ln.out.it), out.view(ln.out.it)):
        bad.append('%s: a second run leaves other bits' % tag)
    bad += ln.findings(tag + ' [second run]')
    if case['B'] > 1 and family == 'normal':
        N = case['Ntok']
        for b in range(case['B']):
            one = Launch(dev, case, t[b:b + 1], B=1)
            one.run()
            bad += one.findings('%s [batch element %d alone]' % (tag, b))
            if not torch.equal(one.out.view.view(ln.out.it), out[b * N:(b + 1) * N].view(ln.out.it)):
                bad.append('%s: batch element %d launched alone leaves other bits than inside the batch' % (tag, b))
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))


def test_attention_refuses_what_it_cannot_run(dev):
    """a head dimension the kernels do not take, a scale that is not positive: refused when the plan runs, nothing is written"""
    case = dict(sm.ATTN_CASES[0])
    for change, fp32, text in ((dict(dhead=6), False, 'multiple of 4'), (dict(dhead=100), True, '<= 96')):
        c = dict(case, fp32=fp32, **change)
        ln = Launch(dev, c, make_qkv(c, 'normal'))
        assert ln.route is None
        with pytest.raises(RuntimeError, match=text):
            ln.run()
        torch.cuda.synchronize()
        assert bool(torch.isnan(ln.out.view).all()) and ln.out.guards_unchanged()
