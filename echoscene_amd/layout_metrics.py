"""Layout metrics of the reference's ``helpers/metrics_3dfront.py`` on the device: the scene-graph constraint accuracy that its
``scripts/eval_3dfront.py`` prints (L/R, F/B, Bi/Sm, Ta/Sh, Stand, Close, Symm, Total) and the box overlap behind its strict rules --
the judge of the layout branch, one step after ``sample_box_and_shape`` -> ``postprocess.descale_box_params``.

``validate_constrains``, ``validate_constrains_changes`` and ``box3d_iou`` take the call shapes of the reference's functions of those
names; the first two append to the same lists in the same order.  The reference walks the triples in Python and fetches two boxes
from the device per triple; here every triple of the call is one thread of one launch (csrc/es_layout_metrics.hip) and the verdicts
come back in one copy.  ``relation_verdicts`` and ``relation_accuracy`` leave the verdicts / the counts per rule on the device side of
that copy, for a whole test set at once: concatenate the scenes with node offsets, as the reference's ``collate_fn`` does; a triple
reads its own two rows only.

Boxes are float32 CUDA tensors [O, 6] or [O, 7], rows (l, h, w, px, py, pz[, angle]): l along z, h along y, w along x, (px, py, pz) the
bottom centre.  The seventh column is ignored: the reference's rules never rotate a box.  The arithmetic is the reference's as numpy 2
evaluates it on float32 boxes, operation by operation (the header of the source file has the details), so verdicts are the
reference's bit for bit wherever its deciding quantity is not within rounding of its threshold.  One deviation: the reference hands
the clipped footprint to ``scipy.spatial.ConvexHull``, which raises on a flat polygon (a box 1 with a zero-size footprint); here that
is area 0 and no error.  Every refusal of the arguments is a ValueError raised before any device work."""
import ctypes as C
import numbers

import numpy as np
import torch

from . import hip

# the accuracy keys of eval in the order of the rule ids, and the predicate names (after the last character is dropped) they answer to
KEYS = ('left', 'right', 'front', 'behind', 'smaller', 'bigger', 'shorter', 'taller', 'standing on', 'close by', 'symmetrical to')
RULE_NAMES = ('left', 'right', 'front', 'behind', 'smaller than', 'bigger than', 'shorter than', 'taller than', 'standing on', 'close by',
              'symmetrical to')
_MODES = {'all': 0, 'unchanged': 1, 'changed': 2}
_KEEP_DTYPES = {torch.float32: 0, torch.int64: 1, torch.bool: 2, torch.uint8: 2, torch.int8: 2, torch.int32: 3}
_AUX = 96                                                           # bytes in front of the verdicts: status int32, counts int32[11][2], padding
_tables = {}


def rule_of_pred(vocab):
    """The rule id of each predicate id of ``vocab['pred_idx_to_name']`` (-1: the predicate has no rule): int8 [n_pred] on the host.
    A name loses its last character, whatever it is, before it is matched, as in the reference (whose vocabulary lines end in a
    newline): 'left\\n' and 'leftX' are the rule ``left``, a bare 'left' is none."""
    return np.array([RULE_NAMES.index(n[:-1]) if n[:-1] in RULE_NAMES else -1 for n in vocab['pred_idx_to_name']], np.int8)


def _check_boxes(who, name, x):
    if not torch.is_tensor(x):
        raise ValueError('%s: %s must be a tensor [O, 6] or [O, 7], got %s' % (who, name, type(x).__name__))
    if x.dtype != torch.float32:
        raise ValueError('%s: %s must be float32, got %s' % (who, name, x.dtype))
    if not (x.dim() == 2 and x.shape[1] in (6, 7) and x.shape[0] > 0):
        raise ValueError('%s: %s must be [O, 6] or [O, 7] with O >= 1, got %s' % (who, name, tuple(x.shape)))
    if x.shape[0] * 7 >= 2 ** 31:
        raise ValueError('%s: %d boxes are beyond int32 indexing' % (who, x.shape[0]))


def _check_devices(who, **tensors):
    """the refusals that come last: one device, and a CUDA device"""
    xs = [(n, x) for n, x in tensors.items() if x is not None]
    for n, x in xs[1:]:
        if x.device != xs[0][1].device:
            raise ValueError('%s: %s is on %s and %s on %s (different devices)' % (who, xs[0][0], xs[0][1].device, n, x.device))
    if not xs[0][1].is_cuda:
        raise ValueError('%s: %s is not on the device (a CUDA tensor is expected)' % (who, xs[0][0]))


def _check(who, triples, boxes, vocab, keep, mode, strict, overlap_threshold):
    """the refusals of the relation calls, in the order: boxes, triples, vocab, keep, mode, strict, overlap_threshold, devices"""
    _check_boxes(who, 'boxes', boxes)
    if not torch.is_tensor(triples):
        raise ValueError('%s: triples must be a tensor [T, 3], got %s' % (who, type(triples).__name__))
    if triples.dtype != torch.int64:
        raise ValueError('%s: triples must be int64, got %s' % (who, triples.dtype))
    if not (triples.dim() == 2 and triples.shape[1] == 3):
        raise ValueError('%s: triples must be [T, 3], got %s' % (who, tuple(triples.shape)))
    if triples.shape[0] >= 2 ** 31 - 256:
        raise ValueError('%s: %d triples are beyond int32 indexing' % (who, triples.shape[0]))
    names = vocab.get('pred_idx_to_name') if isinstance(vocab, dict) else None
    if not (isinstance(names, (list, tuple)) and len(names) > 0 and all(isinstance(n, str) for n in names)):
        raise ValueError("%s: vocab['pred_idx_to_name'] must be a non-empty list of predicate names" % who)
    if keep is not None:
        if not torch.is_tensor(keep):
            raise ValueError('%s: keep must be None or a tensor [O] or [O, 1], got %s' % (who, type(keep).__name__))
        if keep.dtype not in _KEEP_DTYPES:
            raise ValueError('%s: keep must be one of %s, got %s' % (who, sorted(str(d) for d in _KEEP_DTYPES), keep.dtype))
        if tuple(keep.shape) not in ((boxes.shape[0],), (boxes.shape[0], 1)):
            raise ValueError('%s: keep must be [%d] or [%d, 1], one entry per box, got %s' % (who, boxes.shape[0], boxes.shape[0], tuple(keep.shape)))
    if mode not in _MODES:
        raise ValueError('%s: mode must be one of %s, got %r' % (who, sorted(_MODES), mode))
    if not isinstance(strict, (bool, np.bool_)):
        raise ValueError('%s: strict must be a bool, got %r' % (who, strict))
    if not isinstance(overlap_threshold, numbers.Real) or isinstance(overlap_threshold, bool):
        raise ValueError('%s: overlap_threshold must be a real number, got %r' % (who, overlap_threshold))
    _check_devices(who, boxes=boxes, triples=triples, keep=keep)


def _rows(x):
    """x with unit column stride and rows that do not overlap (its row stride is the kernel's leading dimension)"""
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def _rule_table(vocab, dev):
    """rule_of_pred on the device; uploaded once per vocabulary and device"""
    key = (tuple(vocab['pred_idx_to_name']), dev)
    if key not in _tables:
        _tables[key] = torch.from_numpy(rule_of_pred(vocab)).to(dev)
    return _tables[key]


def _launch(triples, boxes, vocab, keep, mode, strict, overlap_threshold, counts):
    """es_relation_check on checked arguments with T >= 1: one uint8 buffer on the device, [status int32 | counts int32[11][2] |
    padding to 96 bytes | rule int8[T] | ok int8[T]], so that everything a caller wants on the host is one copy"""
    dev = boxes.device
    T = triples.shape[0]
    with torch.cuda.device(dev):
        tab = _rule_table(vocab, dev)
        boxes = _rows(boxes)
        triples = triples.contiguous()
        if keep is not None:
            keep = keep.contiguous()
        buf = torch.empty(_AUX + 2 * T, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        hip.check(hip.lib().es_relation_check(
            C.c_void_p(boxes.data_ptr()), boxes.shape[0], boxes.stride(0), C.c_void_p(triples.data_ptr()), T, C.c_void_p(tab.data_ptr()),
            tab.shape[0], hip.ptr(keep), _KEEP_DTYPES[keep.dtype] if keep is not None else 0, _MODES[mode] if keep is not None else 0,
            1 if strict else 0, float(overlap_threshold), C.c_void_p(base + _AUX), C.c_void_p(base + _AUX + T),
            C.c_void_p(base + 4) if counts else None, C.c_void_p(base), hip.current_stream()), 'es_relation_check')
    return buf


def _raise_on_status(who, status, n_boxes, n_pred):
    if status & 1:
        raise ValueError('%s: a triple names a node outside [0, %d)' % (who, n_boxes))
    if status & 2:
        raise ValueError('%s: a triple names a predicate outside [0, %d)' % (who, n_pred))


def _validate(who, mode, triples, pred_boxes, keep, vocab, accuracy, strict, overlap_threshold):
    for k in KEYS + ('total',):
        if not isinstance(accuracy.get(k) if isinstance(accuracy, dict) else None, list):
            raise ValueError('%s: accuracy must be a dict with a list under each of %s' % (who, KEYS + ('total',)))
    _check(who, triples, pred_boxes, vocab, keep, mode, strict, overlap_threshold)
    T = triples.shape[0]
    if T == 0:
        return accuracy
    host = _launch(triples, pred_boxes, vocab, keep, mode, strict, overlap_threshold, False).cpu().numpy()
    _raise_on_status(who, int(host[:4].view(np.int32)[0]), pred_boxes.shape[0], len(vocab['pred_idx_to_name']))
    rule, ok = host[_AUX:_AUX + T].view(np.int8), host[_AUX + T:].view(np.int8)
    for r, v in zip(rule.tolist(), ok.tolist()):
        if r >= 0:
            accuracy[KEYS[r]].append(v)
            accuracy['total'].append(v)
    return accuracy


def validate_constrains(triples, pred_boxes, pred_angles, keep, vocab, accuracy, strict=True, overlap_threshold=0.3):
    """The reference's function of this name: for every triple (s, p, o) of ``triples`` [T, 3] whose predicate has a rule -- with
    ``keep`` given, only those whose two boxes are both kept (``keep == 1``) -- append 1 (fulfilled) or 0 to ``accuracy[<rule key>]``
    and to ``accuracy['total']``, in triple order; returns ``accuracy``.  ``keep`` is None or the [O, 1] / [O] tensor the editing
    calls return; ``pred_angles`` is accepted and unused, as in the reference.  One launch and one copy to the host; T == 0 returns
    ``accuracy`` untouched without a launch.  A triple that names a node or a predicate out of range raises a ValueError after the
    launch (the kernel reads nothing through it) and appends nothing."""
    return _validate('validate_constrains', 'unchanged', triples, pred_boxes, keep, vocab, accuracy, strict, overlap_threshold)


def validate_constrains_changes(triples, pred_boxes, pred_angles, keep, vocab, accuracy, strict=True, overlap_threshold=0.3):
    """The reference's function of this name: as ``validate_constrains``, but with ``keep`` given only the triples with a changed
    box at an end (``keep == 0``) are judged."""
    return _validate('validate_constrains_changes', 'changed', triples, pred_boxes, keep, vocab, accuracy, strict, overlap_threshold)


def relation_verdicts(triples, boxes, vocab, keep=None, mode='all', strict=True, overlap_threshold=0.3):
    """``(rule, ok)``, int8 [T] on the device: the rule id that applied to each triple (the index into ``KEYS``; -1 for a predicate
    without a rule or a triple that ``keep`` leaves out) and whether it is fulfilled (1 / 0; 0 where rule is -1).  ``mode``: 'all'
    judges every triple, 'unchanged' those with both boxes kept, 'changed' those with a box that is not (the selections of
    ``validate_constrains`` and ``validate_constrains_changes``); without ``keep`` every mode is 'all'."""
    _check('relation_verdicts', triples, boxes, vocab, keep, mode, strict, overlap_threshold)
    T = triples.shape[0]
    if T == 0:
        return torch.empty(0, dtype=torch.int8, device=boxes.device), torch.empty(0, dtype=torch.int8, device=boxes.device)
    buf = _launch(triples, boxes, vocab, keep, mode, strict, overlap_threshold, False)
    _raise_on_status('relation_verdicts', int(buf[:4].cpu().numpy().view(np.int32)[0]), boxes.shape[0], len(vocab['pred_idx_to_name']))
    return buf[_AUX:_AUX + T].view(torch.int8), buf[_AUX + T:].view(torch.int8)


def relation_accuracy(triples, boxes, vocab, keep=None, mode='all', strict=True, overlap_threshold=0.3):
    """``{key: (n_ok, n)}`` for the 11 keys of ``KEYS`` and 'total': triples fulfilled and triples judged, counted on the device
    (integer atomics: the counts repeat); 92 bytes come to the host.  Arguments as ``relation_verdicts``; ``summarize`` turns the
    result into the row eval prints."""
    _check('relation_accuracy', triples, boxes, vocab, keep, mode, strict, overlap_threshold)
    if triples.shape[0] == 0:
        cnt = np.zeros((len(KEYS), 2), np.int64)
    else:
        aux = _launch(triples, boxes, vocab, keep, mode, strict, overlap_threshold, True)[:_AUX].cpu().numpy().view(np.int32)
        _raise_on_status('relation_accuracy', int(aux[0]), boxes.shape[0], len(vocab['pred_idx_to_name']))
        cnt = aux[1:1 + 2 * len(KEYS)].reshape(len(KEYS), 2).astype(np.int64)
    out = {k: (int(cnt[r, 0]), int(cnt[r, 1])) for r, k in enumerate(KEYS)}
    out['total'] = (int(cnt[:, 0].sum()), int(cnt[:, 1].sum()))
    return out


def summarize(accuracy_or_counts):
    """The row that eval prints, from the accuracy lists of the ``validate_constrains`` calls or from the ``{key: (n_ok, n)}`` counts
    of ``relation_accuracy``: 'L/R', 'F/B', 'Bi/Sm', 'Ta/Sh' are the means of the two rules' means, 'Stand', 'Close', 'Symm', 'Total'
    plain means, 'means of mean' the mean of the first seven.  Host, float64; a rule without a triple is NaN, as ``np.mean([])``."""
    a = accuracy_or_counts
    if not isinstance(a, dict) or any(k not in a for k in KEYS + ('total',)):
        raise ValueError('summarize: expects a dict with the keys %s' % (KEYS + ('total',),))

    def mean(k):
        v = a[k]
        if isinstance(v, tuple):
            n_ok, n = v
            return float(n_ok) / float(n) if n else float('nan')
        return float(np.mean(np.asarray(v, np.float64))) if len(v) else float('nan')

    m = [mean(k) for k in KEYS]
    row = {'L/R': (m[0] + m[1]) / 2, 'F/B': (m[2] + m[3]) / 2, 'Bi/Sm': (m[4] + m[5]) / 2, 'Ta/Sh': (m[6] + m[7]) / 2, 'Stand': m[8],
           'Close': m[9], 'Symm': m[10]}
    row['Total'] = mean('total')
    row['means of mean'] = float(np.mean([row[k] for k in ('L/R', 'F/B', 'Bi/Sm', 'Ta/Sh', 'Stand', 'Close', 'Symm')]))
    return row


def box3d_iou(box1, box2, param6=True, with_translation=False):
    """The reference's ``box3d_iou`` for K pairs of boxes at once: ``box1`` and ``box2`` are float32 CUDA tensors [K, 6] or [K, 7] (a
    single row [6] or [7] is K = 1) -> ``(iou, iou_2d)``, float64 [K] on the device: the volume of the intersection over the smaller of
    the two volumes, and the intersection over the union of the footprints.  No rotation; ``param6`` is accepted and ignored (the width
    of the rows says it); ``with_translation=False`` centres both boxes at the origin.  Touching boxes, and a ``box2`` whose footprint
    is flat or negatively wound (l * w <= 0), intersect in nothing; a zero volume gives 0 / 0 = NaN."""
    if torch.is_tensor(box1) and box1.dim() == 1:
        box1 = box1[None]
    if torch.is_tensor(box2) and box2.dim() == 1:
        box2 = box2[None]
    _check_boxes('box3d_iou', 'box1', box1)
    _check_boxes('box3d_iou', 'box2', box2)
    if box1.shape[0] != box2.shape[0]:
        raise ValueError('box3d_iou: %d rows in box1 and %d in box2 (pairs are taken row by row)' % (box1.shape[0], box2.shape[0]))
    _check_devices('box3d_iou', box1=box1, box2=box2)
    K = box1.shape[0]
    with torch.cuda.device(box1.device):
        a, b = _rows(box1), _rows(box2)
        out = torch.empty(2, K, dtype=torch.float64, device=a.device)
        hip.check(hip.lib().es_box3d_iou(C.c_void_p(a.data_ptr()), a.stride(0), C.c_void_p(b.data_ptr()), b.stride(0), K,
                                         1 if with_translation else 0, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
                                         hip.current_stream()), 'es_box3d_iou')
    return out[0], out[1]
