"""Host yardsticks and seeded cases of the layout-metric tests (echoscene_amd/layout_metrics.py, csrc/es_layout_metrics.hip).

Three things, all numpy / pure Python:
  * a restatement of the relation rules and of the box IoU in the arithmetic the kernel promises: the fp32 rules with numpy float32
    scalars (one rounding per operation, thresholds rounded to float32), the corner rules in float64 with sequential sums
    (``check``, ``box3d_iou``);
  * an exact yardstick for the two IoUs with ``fractions.Fraction`` (the boxes are float32, the intersection of two axis-aligned
    rectangles is rational), and the exact distance of each verdict's deciding quantity to its threshold (``iou_exact``, ``margin``);
  * the case builders that the golden generator (tests/golden/make_golden_layout_metrics.py) and the tests share (``CASES``, ``case``).

Boxes are rows (l, h, w, px, py, pz[, angle]): l along z, h along y, w along x, (px, py, pz) the bottom centre."""
import math
from fractions import Fraction

import numpy as np

KEYS = ('left', 'right', 'front', 'behind', 'smaller', 'bigger', 'shorter', 'taller', 'standing on', 'close by', 'symmetrical to')
ALL_KEYS = KEYS + ('total',)
RULE_NAMES = ('left', 'right', 'front', 'behind', 'smaller than', 'bigger than', 'shorter than', 'taller than', 'standing on', 'close by',
              'symmetrical to')
LEFT, RIGHT, FRONT, BEHIND, SMALLER, BIGGER, SHORTER, TALLER, STAND, CLOSE, SYMM = range(11)
# 16 predicates, five of them without a rule; every name ends in the newline of a vocabulary file
PRED_NAMES = ('none', 'left', 'right', 'front', 'behind', 'close by', 'symmetrical to', 'bigger than', 'smaller than', 'taller than',
              'shorter than', 'standing on', 'same material as', 'same style as', 'same super category as', 'inside')
VOCAB = {'pred_idx_to_name': [n + '\n' for n in PRED_NAMES]}
PRED_OF_RULE = [PRED_NAMES.index(n) for n in RULE_NAMES]
F = np.float32


def rule_of_pred(vocab):
    """rule id per predicate id, -1 for none; the last character of a name is dropped, whatever it is"""
    return np.array([RULE_NAMES.index(n[:-1]) if n[:-1] in RULE_NAMES else -1 for n in vocab['pred_idx_to_name']], np.int8)


def empty_accuracy():
    return {k: [] for k in ALL_KEYS}


# ------------------------------------------------------------------------------------------------ the restatement
def corners(box, with_translation):
    """z and x of corners 0..3, top, bottom: the halves in float32, the sums in float64"""
    l, h, w, px, py, pz = (F(v) for v in box[:6])
    hl, hw = l / F(2), w / F(2)
    tx, ty, tz = (float(px), float(py), float(pz)) if with_translation else (0.0, 0.0, 0.0)
    z = [float(hl) + tz, float(-hl) + tz, float(-hl) + tz, float(hl) + tz]
    x = [float(hw) + tx, float(hw) + tx, float(-hw) + tx, float(-hw) + tx]
    return z, x, float(h) + ty, 0.0 + ty


def _shoelace(u, v):
    p = q = 0.0
    for i in range(len(u)):
        p += u[i] * v[i - 1]
        q += v[i] * u[i - 1]
    return 0.5 * abs(p - q)


def _clip(subject, clip):
    """Sutherland-Hodgman with the strict inside test; None when nothing is left"""
    out = subject
    cp1 = clip[-1]
    for cp2 in clip:
        inp, out = out, []
        s = inp[-1]
        for e in inp:
            e_in = (cp2[0] - cp1[0]) * (e[1] - cp1[1]) > (cp2[1] - cp1[1]) * (e[0] - cp1[0])
            s_in = (cp2[0] - cp1[0]) * (s[1] - cp1[1]) > (cp2[1] - cp1[1]) * (s[0] - cp1[0])
            if e_in != s_in:
                dc = (cp1[0] - cp2[0], cp1[1] - cp2[1])
                dp = (s[0] - e[0], s[1] - e[1])
                n1 = cp1[0] * cp2[1] - cp1[1] * cp2[0]
                n2 = s[0] * e[1] - s[1] * e[0]
                n3 = 1.0 / (dc[0] * dp[1] - dc[1] * dp[0])
                out.append(((n1 * dp[0] - n2 * dc[0]) * n3, (n1 * dp[1] - n2 * dc[1]) * n3))
            if e_in:
                out.append(e)
            s = e
        cp1 = cp2
        if not out:
            return None
    return out


def _div(a, b):
    """IEEE quotient of two Python floats (0 / 0 = NaN, x / 0 = inf)"""
    with np.errstate(all='ignore'):
        return float(np.float64(a) / np.float64(b))


def box3d_iou(box1, box2, with_translation=False):
    """(iou, iou_2d) as Python floats; NaN where a volume or both areas are zero"""
    z1, x1, top1, bot1 = corners(box1, with_translation)
    z2, x2, top2, bot2 = corners(box2, with_translation)
    a1, a2 = _shoelace(z1, x1), _shoelace(z2, x2)
    poly = _clip(list(zip(z1, x1)), list(zip(z2, x2)))
    inter = 0.0 if poly is None else _shoelace([p[0] for p in poly], [p[1] for p in poly])
    iou_2d = _div(inter, a1 + a2 - inter)
    ymax = top2 if top2 < top1 else top1
    ymin = bot2 if bot2 > bot1 else bot1
    dy = ymax - ymin
    inter_vol = inter * (dy if dy > 0.0 else 0.0)

    def vol(z, x, top, bot):
        dz, dx, dh = z[0] - z[1], x[1] - x[2], top - bot
        return math.sqrt(dz * dz) * math.sqrt(dx * dx) * math.sqrt(dh * dh)
    v1, v2 = vol(z1, x1, top1, bot1), vol(z2, x2, top2, bot2)
    return _div(inter_vol, v2 if v2 < v1 else v1), iou_2d


def _closest(s, o):
    zs, xs, tops, bots = corners(s, True)
    zo, xo, topo, boto = corners(o, True)
    best, nan = math.inf, False
    for i in range(8):
        for j in range(8):
            dx, dy, dz = xs[i & 3] - xo[j & 3], (tops if i < 4 else bots) - (topo if j < 4 else boto), zs[i & 3] - zo[j & 3]
            d = math.sqrt(dx * dx + dy * dy + dz * dz)
            nan |= d != d
            best = d if d < best else best
    return math.nan if nan else best


def verdict(rule, s, o, strict=True, overlap_threshold=0.3):
    """1 / 0 for one triple whose predicate has rule ``rule``"""
    s, o = np.asarray(s, F), np.asarray(o, F)
    with np.errstate(all='ignore'):
        if rule <= BEHIND:
            d = s[5] - o[5] if rule in (LEFT, RIGHT) else s[3] - o[3]
            fail = bool({LEFT: d > F(-0.05), RIGHT: d < F(0.05), FRONT: d < F(-0.05), BEHIND: d > F(0.05)}[rule])
            if not fail and strict:
                fail = box3d_iou(s, o, True)[0] > overlap_threshold
            return int(not fail)
        if rule in (SMALLER, BIGGER):
            vs, vo = s[0] * s[1] * s[2], o[0] * o[1] * o[2]
            q = (vs - vo) / vs
            return int(not (q < F(0.15))) if rule == BIGGER else int(not (q > F(-0.15)))
        if rule in (SHORTER, TALLER):
            hs, ho = s[4] + s[1], o[4] + o[1]
            q = (hs - ho) / hs
            return int(not (q < F(0.1))) if rule == TALLER else int(not (q > F(-0.1)))
        if rule == STAND:
            return int(bool(np.abs(s[4] - o[4]) < F(0.04)))
        if rule == CLOSE:
            return int(not (_closest(s, o) > 0.45))

        def l2(p1, p2):
            dx, dz = p2[0] - p1[0], p2[1] - p1[1]
            return np.sqrt(dx * dx + dz * dz)
        oc = (o[3], o[5])
        return int(bool(l2((-s[3], -s[5]), oc) < F(0.45) or l2((-s[3], s[5]), oc) < F(0.45) or l2((s[3], -s[5]), oc) < F(0.45)))


def taken(keep, mode, s, o):
    """does the keep mask let the triple through ('all', 'unchanged': both ends kept, 'changed': an end not kept)"""
    if keep is None or mode == 'all':
        return True
    k = np.asarray(keep).reshape(-1)
    return bool(k[s] == 1 and k[o] == 1) if mode == 'unchanged' else bool(k[s] == 0 or k[o] == 0)


def check(triples, boxes, vocab=VOCAB, keep=None, mode='all', strict=True, overlap_threshold=0.3):
    """(rule int8 [T], ok int8 [T]) as the kernel writes them"""
    tab = rule_of_pred(vocab)
    rule, ok = np.full(len(triples), -1, np.int8), np.zeros(len(triples), np.int8)
    for t, (s, p, o) in enumerate(np.asarray(triples).tolist()):
        if tab[p] >= 0 and taken(keep, mode, s, o):
            rule[t] = tab[p]
            ok[t] = verdict(int(tab[p]), boxes[s], boxes[o], strict, overlap_threshold)
    return rule, ok


def accuracy_of(rule, ok, accuracy=None):
    """the lists the drop-in functions append, from the verdict arrays"""
    accuracy = empty_accuracy() if accuracy is None else accuracy
    for r, v in zip(np.asarray(rule).tolist(), np.asarray(ok).tolist()):
        if r >= 0:
            accuracy[KEYS[r]].append(v)
            accuracy['total'].append(v)
    return accuracy


def summary_row(accuracy):
    """the row of eval from the lists, by the formulas (np.mean of an empty list is NaN)"""
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m = [np.mean(accuracy[k]) for k in ALL_KEYS]
            row = {'L/R': np.mean([m[0], m[1]]), 'F/B': np.mean([m[2], m[3]]), 'Bi/Sm': np.mean([m[4], m[5]]),
                   'Ta/Sh': np.mean([m[6], m[7]]), 'Stand': m[8], 'Close': m[9], 'Symm': m[10]}
            row['means of mean'] = np.mean(list(row.values()))
            row['Total'] = m[11]
    return {k: float(v) for k, v in row.items()}


# ------------------------------------------------------------------------------------------------ the exact yardstick
def _fr(v):
    return Fraction(float(F(v)))


def iou_exact(box1, box2, with_translation=False):
    """(iou, iou_2d) as Fractions, None where the value is 0 / 0.  The footprint of box 2 clips only when it is wound counter-clockwise
    (l * w > 0); the clip is strict, so touching footprints share nothing -- which is their exact common area too."""
    l1, h1, w1, px1, py1, pz1 = (_fr(v) for v in box1[:6])
    l2, h2, w2, px2, py2, pz2 = (_fr(v) for v in box2[:6])
    if not with_translation:
        px1 = py1 = pz1 = px2 = py2 = pz2 = Fraction(0)

    def span(c, size):
        return c - abs(size) / 2, c + abs(size) / 2
    inter = Fraction(0)
    if l2 * w2 > 0:
        (za, zb), (zc, zd) = span(pz1, l1), span(pz2, l2)
        (xa, xb), (xc, xd) = span(px1, w1), span(px2, w2)
        inter = max(Fraction(0), min(zb, zd) - max(za, zc)) * max(Fraction(0), min(xb, xd) - max(xa, xc))
    a1, a2 = abs(l1 * w1), abs(l2 * w2)
    union = a1 + a2 - inter
    iou_2d = inter / union if union != 0 else None
    dy = max(Fraction(0), min(h1 + py1, h2 + py2) - max(py1, py2))
    vmin = min(a1 * abs(h1), a2 * abs(h2))
    return (inter * dy / vmin if vmin != 0 else None), iou_2d


def margin(rule, s, o, strict=True, overlap_threshold=0.3):
    """the distance of the deciding quantity of a verdict to its threshold, from exact arithmetic on the float32 boxes (roots in
    float64).  A strict rule that already fails on the centres is decided there; one that passes them is decided by both the centres
    and the IoU.  A quantity that is 0 / 0 decides nothing (NaN compares false whatever the rounding): inf."""
    s, o = [_fr(v) for v in s[:6]], [_fr(v) for v in o[:6]]
    thr32 = lambda v: Fraction(float(F(v)))
    if rule <= BEHIND:
        d = s[5] - o[5] if rule in (LEFT, RIGHT) else s[3] - o[3]
        t = thr32({LEFT: -0.05, RIGHT: 0.05, FRONT: -0.05, BEHIND: 0.05}[rule])
        fail = {LEFT: d > t, RIGHT: d < t, FRONT: d < t, BEHIND: d > t}[rule]
        m = abs(d - t)
        if not fail and strict:
            iou = iou_exact([float(v) for v in s], [float(v) for v in o], True)[0]
            if iou is not None:
                m = min(m, abs(iou - Fraction(overlap_threshold)))
        return float(m)
    if rule in (SMALLER, BIGGER, SHORTER, TALLER):
        a, b = (s[0] * s[1] * s[2], o[0] * o[1] * o[2]) if rule in (SMALLER, BIGGER) else (s[4] + s[1], o[4] + o[1])
        if a == 0:
            return math.inf
        t = thr32({SMALLER: -0.15, BIGGER: 0.15, SHORTER: -0.1, TALLER: 0.1}[rule])
        return float(abs((a - b) / a - t))
    if rule == STAND:
        return float(abs(abs(s[4] - o[4]) - thr32(0.04)))
    if rule == CLOSE:
        best = math.inf
        for xs in (s[3] + s[2] / 2, s[3] - s[2] / 2):
            for ys in (s[4] + s[1], s[4]):
                for zs in (s[5] + s[0] / 2, s[5] - s[0] / 2):
                    for xo in (o[3] + o[2] / 2, o[3] - o[2] / 2):
                        for yo in (o[4] + o[1], o[4]):
                            for zo in (o[5] + o[0] / 2, o[5] - o[0] / 2):
                                best = min(best, math.sqrt(float((xs - xo) ** 2 + (ys - yo) ** 2 + (zs - zo) ** 2)))
        return abs(best - 0.45)
    t = float(thr32(0.45))
    return min(abs(math.sqrt(float((o[3] - a) ** 2 + (o[5] - b) ** 2)) - t)
               for a, b in ((-s[3], -s[5]), (-s[3], s[5]), (s[3], -s[5])))


def margins(c):
    """margin of every judged triple of a case (both keep selections), as a list"""
    tab = rule_of_pred(VOCAB)
    return [margin(int(tab[p]), c['boxes'][s], c['boxes'][o], c['strict'], c['overlap_threshold'])
            for s, p, o in c['triples'].tolist() if tab[p] >= 0]


# ------------------------------------------------------------------------------------------------ the cases
def random_scene(seed, O=12, T=120, cols=6):
    """sizes uniform in 0.2 .. 2, centres in +-2.5, predicates 0 .. 15, subject != object"""
    rs = np.random.RandomState(seed)
    boxes = np.concatenate([rs.uniform(0.2, 2.0, (O, 3)), rs.uniform(-2.5, 2.5, (O, 3))], 1).astype(F)
    if cols == 7:
        boxes = np.concatenate([boxes, rs.uniform(-180, 180, (O, 1)).astype(F)], 1)
    s = rs.randint(0, O, T)
    o = (s + rs.randint(1, O, T)) % O
    return boxes, np.stack([s, rs.randint(0, len(PRED_NAMES), T), o], 1).astype(np.int64)


def _pairs(rows):
    """[(rule, subject box, object box)] -> boxes [2 n, 6], triples [n, 3]"""
    boxes, triples = [], []
    for rule, s, o in rows:
        triples.append((len(boxes), PRED_OF_RULE[rule], len(boxes) + 1))
        boxes += [s, o]
    return np.array(boxes, F), np.array(triples, np.int64)


def planted():
    """every rule x outcome, and for the four strict rules also "fails only because of the overlap": a small box inside a large one
    on the right side of it (the IoU is over the smaller volume, so it is 1)"""
    big = lambda x, z: [2.0, 2.0, 2.0, x, 0.0, z]
    small = lambda x, z: [0.3, 0.3, 0.3, x, 0.1, z]
    unit = lambda x, y, z, k=1.0: [k, k, k, x, y, z]
    rows = []
    for rule, axis, sign in ((LEFT, 'z', -1), (RIGHT, 'z', 1), (FRONT, 'x', 1), (BEHIND, 'x', -1)):
        xz = (lambda v: (0.0, v)) if axis == 'z' else (lambda v: (v, 0.0))          # a position along the rule's axis, `sign` the right side
        half = lambda v: [0.5, 0.5, 0.5, xz(v)[0], 0.0, xz(v)[1]]
        rows += [(rule, half(sign * 1.5), half(-sign * 1.5)),                       # fulfilled, far apart
                 (rule, half(-sign * 1.5), half(sign * 1.5)),                       # the wrong side
                 (rule, small(*xz(sign * 0.25)), big(0.0, 0.0)),                    # the right side, but inside: the overlap alone fails it
                 (rule, unit(xz(sign * 0.75)[0], 0.0, xz(sign * 0.75)[1]), unit(0.0, 0.0, 0.0))]      # overlap 1/4, below 0.3
    rows += [(BIGGER, unit(0, 0, 0, 1.0), unit(2, 0, 0, 0.5)), (BIGGER, unit(0, 0, 0, 0.5), unit(2, 0, 0, 1.0)),
             (BIGGER, unit(0, 0, 0, 1.0), unit(2, 0, 0, 0.97)),                                                     # bigger, but by less than 15 %
             (SMALLER, unit(0, 0, 0, 0.5), unit(2, 0, 0, 1.0)), (SMALLER, unit(0, 0, 0, 1.0), unit(2, 0, 0, 0.5)),
             (SMALLER, unit(0, 0, 0, 0.97), unit(2, 0, 0, 1.0)),
             (TALLER, [1, 1.5, 1, 0, 0, 0], [1, 0.5, 1, 2, 0, 0]), (TALLER, [1, 0.5, 1, 0, 0, 0], [1, 1.5, 1, 2, 0, 0]),
             (TALLER, [1, 0.5, 1, 0, 1.0, 0], [1, 1.0, 1, 2, 0, 0]),                                                # lower box, higher top
             (SHORTER, [1, 0.5, 1, 0, 0, 0], [1, 1.5, 1, 2, 0, 0]), (SHORTER, [1, 1.5, 1, 0, 0, 0], [1, 0.5, 1, 2, 0, 0]),
             (SHORTER, [1, 1.0, 1, 0, 0, 0], [1, 1.05, 1, 2, 0, 0]),
             (STAND, unit(0, 0.0, 0), unit(2, 0.01, 0)), (STAND, unit(0, 0.5, 0), unit(0, 0.0, 0)), (STAND, unit(0, -0.03, 0), unit(2, 0.0, 0)),
             (CLOSE, unit(0, 0, 0), unit(1.2, 0, 0)), (CLOSE, unit(0, 0, 0), unit(3, 0, 0)), (CLOSE, unit(0, 0, 0), unit(1.0, 1.3, 0)),
             (CLOSE, unit(0, 0, 0, 0.5), unit(0, 0, 0, 2.0)),                                                       # nested: the corners are far apart
             (SYMM, unit(1, 0, 1), unit(-1, 0, -1)), (SYMM, unit(1, 0, 1), unit(-1.2, 0, 1.1)), (SYMM, unit(1, 0, 1), unit(0.8, 0, -1)),
             (SYMM, unit(1, 0, 1), unit(2, 0, 0.3)), (SYMM, unit(1, 0, 1), unit(1, 0, 1))]
    return _pairs(rows)


def self_triples():
    """every predicate with the subject as its own object"""
    boxes, _ = random_scene(11, O=3)
    return boxes, np.array([(n % 3, p, n % 3) for n, p in enumerate(range(len(PRED_NAMES)))], np.int64)


def negative_sizes():
    """negative sizes at either end of a strict rule whose centres pass (the overlap decides), and of the size rules"""
    rows = []
    for rule, x, z in ((LEFT, 0.0, -0.25), (RIGHT, 0.0, 0.25), (FRONT, 0.25, 0.0), (BEHIND, -0.25, 0.0)):
        rows += [(rule, [-0.3, 0.3, 0.3, x, 0.1, z], [2, 2, 2, 0, 0, 0]),          # box 1 wound clockwise: clips as usual
                 (rule, [-0.3, 0.3, -0.3, x, 0.1, z], [2, 2, 2, 0, 0, 0]),
                 (rule, [0.3, 0.3, 0.3, x, 0.1, z], [-2, 2, 2, 0, 0, 0]),          # box 2 wound clockwise: nothing is inside it
                 (rule, [0.3, 0.3, 0.3, x, 0.1, z], [-2, 2, -2, 0, 0, 0]),         # both signs flipped: counter-clockwise again
                 (rule, [0.3, -0.3, 0.3, x, 0.4, z], [2, 2, 2, 0, 0, 0]),          # negative height: the top is below the bottom
                 (rule, [0.3, 0.3, 0.3, x, 0.1, z], [2, -2, 2, 0, 2, 0])]
    rows += [(BIGGER, [-1, 1, 1, 0, 0, 0], [0.5, 0.5, 0.5, 2, 0, 0]), (SMALLER, [-1, 1, 1, 0, 0, 0], [0.5, 0.5, 0.5, 2, 0, 0]),
             (BIGGER, [1, 1, 1, 0, 0, 0], [-0.5, 0.5, 0.5, 2, 0, 0]), (TALLER, [1, -1.5, 1, 0, 1, 0], [1, 0.5, 1, 2, 0, 0]),
             (SHORTER, [1, -1.5, 1, 0, 1, 0], [1, 0.5, 1, 2, 0, 0]), (CLOSE, [-1, 1, -1, 0, 0, 0], [1, -1, 1, 1.2, 0, 0]),
             (CLOSE, [-1, 1, -1, 0, 0, 0], [1, 1, 1, 3, 0, 0])]
    return _pairs(rows)


def flat_box2():
    """a box 2 without footprint or without height under a strict rule whose centres pass: the IoU is 0 / 0 = NaN, not above any
    threshold"""
    rows = []
    for rule, x, z in ((LEFT, 0.0, -0.25), (RIGHT, 0.0, 0.25), (FRONT, 0.25, 0.0), (BEHIND, -0.25, 0.0)):
        rows += [(rule, [0.3, 0.3, 0.3, x, 0.1, z], [2, 2, 0, 0, 0, 0]), (rule, [0.3, 0.3, 0.3, x, 0.1, z], [0, 2, 2, 0, 0, 0]),
                 (rule, [0.3, 0.3, 0.3, x, 0.1, z], [2, 0, 2, 0, 0, 0])]
    return _pairs(rows)


def threshold_edges():
    """the fp32 thresholds hit exactly and missed by one ulp on either side: the centre differences against +-0.05, |dy| against 0.04,
    the flipped-centre distance against 0.45 (the other coordinate 0, so the root returns |dx|).  The object sits at 0 in the
    deciding coordinate, so the difference is the subject's coordinate; the strict rules' boxes are 5 apart on the other axis"""
    rows = []

    def around(v):
        v = F(v)
        return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]
    for rule, t in ((LEFT, -0.05), (RIGHT, 0.05), (FRONT, -0.05), (BEHIND, 0.05)):
        for v in around(t):
            s = [1, 1, 1, 5, 0, v] if rule in (LEFT, RIGHT) else [1, 1, 1, v, 0, 5]
            rows.append((rule, s, [1, 1, 1, 0, 0, 0]))
    for t in (0.04, -0.04):
        rows += [(STAND, [1, 1, 1, 0, v, 0], [1, 1, 1, 2, 0, 0]) for v in around(t)]
    for t in (0.45, -0.45):
        rows += [(SYMM, [1, 1, 1, 0, 0, 0], [1, 1, 1, v, 0, 0]) for v in around(t)]
        rows += [(SYMM, [1, 1, 1, 0, 0, 0], [1, 1, 1, 0, 0, v]) for v in around(t)]
    return _pairs(rows)


def _keep_mask(seed, O):
    return (np.random.RandomState(seed).uniform(size=(O, 1)) < 0.6).astype(F)


# name -> (builder, seed of the keep mask or None, strict, overlap_threshold, the drop-in functions recorded).  The reference's
# validate_constrains_changes passes 7-column boxes to a 6-column unpacking, so 7 columns are recorded through validate_constrains alone.
BOTH = ('validate_constrains', 'validate_constrains_changes')
CASES = {
    'random0': (lambda: random_scene(100), None, True, 0.3, BOTH),
    'random1': (lambda: random_scene(101), None, True, 0.3, BOTH),
    'random2': (lambda: random_scene(102), None, True, 0.3, BOTH),
    'random_thr': (lambda: random_scene(103), None, True, 0.05, BOTH),
    'planted': (planted, None, True, 0.3, BOTH),
    'planted_loose': (planted, None, False, 0.3, BOTH),
    'keep': (lambda: random_scene(104), 5, True, 0.3, BOTH),
    'keep_planted': (planted, 6, True, 0.3, BOTH),
    'cols7': (lambda: random_scene(105, cols=7), None, True, 0.3, BOTH[:1]),
    'self': (self_triples, None, True, 0.3, BOTH),
    'negative': (negative_sizes, None, True, 0.3, BOTH),
    'flat2': (flat_box2, None, True, 0.3, BOTH),
    'edges': (threshold_edges, None, True, 0.3, BOTH),
}
MODE_OF = {'validate_constrains': 'unchanged', 'validate_constrains_changes': 'changed'}


def case(name):
    build, keep, strict, thr, fns = CASES[name]
    boxes, triples = build()
    return {'boxes': boxes, 'triples': triples, 'keep': None if keep is None else _keep_mask(keep, len(boxes)), 'strict': strict,
            'overlap_threshold': thr, 'functions': fns}


def iou_pairs():
    """(box1 [K, 6], box2 [K, 6], with_translation) sets whose IoUs the generator records: every (s, o) of the planted, negative-size
    and flat cases and of a random scene with translation, and the random scene's without (every pair overlaps then)"""
    out = []
    for name in ('planted', 'negative', 'flat2', 'self', 'random0'):
        c = case(name)
        s, o = c['triples'][:, 0], c['triples'][:, 2]
        out.append((c['boxes'][s, :6], c['boxes'][o, :6], True))
    c = case('random1')
    out.append((c['boxes'][c['triples'][:, 0], :6], c['boxes'][c['triples'][:, 2], :6], False))
    return out


def tiny(T, seed=0):
    """O = 2 and T triples over every predicate and both directions (and s == o)"""
    boxes = np.array([[0.8, 1.0, 0.6, 0.3, 0.0, -0.4], [1.1, 0.5, 0.9, -0.2, 0.02, 0.35]], F)
    rs = np.random.RandomState(seed + T)
    return boxes, np.stack([rs.randint(0, 2, T), rs.randint(0, len(PRED_NAMES), T), rs.randint(0, 2, T)], 1).astype(np.int64)


CHAIN_STATS = np.array([0.2, 0.25, 0.3, 2.0, 2.5, 1.8, -2.5, 0.0, -3.0, 2.5, 1.5, 3.0], np.float64)     # size minima, maxima; centre minima, maxima


def chain_case(seed=7, O=12, T=120):
    """normalised boxes in [-1, 1] and the statistics that ``postprocess.descale_box_params`` takes them back with; triples as
    ``random_scene``"""
    rs = np.random.RandomState(seed)
    _, triples = random_scene(seed, O, T)
    return rs.uniform(-1, 1, (O, 6)).astype(F), CHAIN_STATS, triples


def descale(normed, stats):
    """descale_box_params in float32, operation by operation: (v + 1) / 2 * (hi - lo) + lo"""
    st = np.asarray(stats, F)
    lo, hi = np.concatenate([st[0:3], st[6:9]]), np.concatenate([st[3:6], st[9:12]])
    return ((np.asarray(normed, F) + F(1)) / F(2) * (hi - lo) + lo).astype(F)
