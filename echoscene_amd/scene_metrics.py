"""The scene-level metric of the reference's ``helpers/metrics_3dfront.py`` on the device: how far shapes placed in their boxes run into
each other (``pointcloud_overlap``), one step after ``sample_box_and_shape`` -> ``sdf_to_mesh`` -> ``shape_metrics.point_clouds``.

``fit_shapes_to_box``, ``pointcloud_overlap_pair`` and ``pointcloud_overlap`` take the call shapes of the reference's functions of those
names (``helpers/util.py`` for the first); ``pointcloud_overlap`` appends to the same list in the same order.  The reference works pair
by pair on the host: two copies from the device, a numpy fit and a scikit-learn kd-tree per pair.  Here a call is three launches
(csrc/es_scene_metrics.hip): the fit of every cloud, one nearest-neighbour pass of every cloud over itself, and one pass per pair that
a bounding-box test cuts short; ``overlap_counts`` does that for a whole test set and leaves the counts on the device.

The count of a pair (first cloud, second cloud): a point ``p`` of the first cloud counts 1 when its nearest point of the second cloud is
STRICTLY nearer than its nearest OTHER point of the first cloud (another index: a duplicate of ``p`` is at distance 0 and wins), else 0.
Distances are ``dx*dx + dy*dy + dz*dz`` in fp32 from direct differences, summed in that order, nothing fused, compared as squares.  A
first cloud of one point has no other point: it counts.  This is the reference's number wherever that is defined (its query finds the
point itself at distance 0 in one of the two neighbour slots; a point of the second cloud coincident with ``p`` counts on both sides).
One deviation: on an exact tie between the two distances the reference follows the visiting order of its kd-tree; here the own cloud
wins and the point counts 0.

The fit runs per axis in fp32, in the reference's order: ``size = max - min`` over the cloud, ``p / size * box[:3]``, the rotation by
``box[6]`` degrees, ``+ box[3:6]``.  ``up='z'`` turns about z as the reference's ``get_rotation`` (x' = c x - s y, y' = s x + c y), which is
what the reference's metric does; ``up='y'`` turns about y as its ``get_rotation_3dfront`` (x' = c x - s z, z' = s x + c z), the convention
of every box this package returns.  The radians are fp32 (numpy's ``deg2rad`` on a float32), the cosine and sine the correctly rounded
fp32 values.  A cloud without extent along an axis (the reference divides by zero) or a value that is not finite (its kd-tree refuses
it) raises.

Inputs are CUDA tensors; every cloud of a call has the same number of points.  Every refusal of the arguments is a ValueError raised
before any device work; what only the device can see (a flat cloud, a NaN, a pair index out of range) is a ValueError after it."""
import ctypes as C

import numpy as np
import torch

from . import hip
from .layout_metrics import _check_devices, _rows            # one device and a CUDA device; rows with unit column stride

STRUCTURAL = ('floor', 'wall', 'ceiling', '_scene_')
TOUCHING = ('none', 'inside', 'attached to', 'part of', 'cover', 'belonging to', 'build in', 'connected to')
_UP = {'z': 0, 'y': 1}


# ------------------------------------------------------------------------------------------------ refusals
def _check_up(who, up):
    if up not in _UP:
        raise ValueError("%s: up must be 'z' or 'y', got %r" % (who, up))


def _check_clouds(who, name, x):
    if not torch.is_tensor(x):
        raise ValueError('%s: %s must be a tensor [O, P, 3], got %s' % (who, name, type(x).__name__))
    if x.dtype != torch.float32:
        raise ValueError('%s: %s must be float32, got %s' % (who, name, x.dtype))
    if not (x.dim() == 3 and x.shape[2] == 3 and x.shape[0] > 0 and x.shape[1] > 0):
        raise ValueError('%s: %s must be [O, P, 3] with O >= 1 and P >= 1, got %s' % (who, name, tuple(x.shape)))
    if x.numel() >= 2 ** 31 - 1:
        raise ValueError('%s: %s with %d values is beyond int32 indexing' % (who, name, x.numel()))


def _check_boxes(who, boxes, O, withangle):
    if not torch.is_tensor(boxes):
        raise ValueError('%s: boxes must be a tensor [O, 7] or [O, 6], got %s' % (who, type(boxes).__name__))
    if boxes.dtype != torch.float32:
        raise ValueError('%s: boxes must be float32, got %s' % (who, boxes.dtype))
    cols = (7,) if withangle else (6, 7)
    if not (boxes.dim() == 2 and boxes.shape[1] in cols):
        raise ValueError('%s: boxes must be [O, %s]%s, got %s' % (who, ' or '.join(str(c) for c in cols),
                                                                  ' (the angle is the seventh column)' if withangle else '', tuple(boxes.shape)))
    if boxes.shape[0] != O:
        raise ValueError('%s: %d boxes for %d clouds' % (who, boxes.shape[0], O))


def _check_cloud_list(who, pclouds):
    """a tensor [O, P, 3], or a list of O tensors [P, 3] with one common P -> the tensor, or the list as it is (stacked after every
    refusal: a copy on the device, no arithmetic)"""
    if torch.is_tensor(pclouds):
        _check_clouds(who, 'pclouds', pclouds)
        return pclouds
    if not (isinstance(pclouds, (list, tuple)) and len(pclouds) > 0 and all(torch.is_tensor(p) for p in pclouds)):
        raise ValueError('%s: pclouds must be a tensor [O, P, 3] or a non-empty list of tensors [P, 3]' % who)
    for n, p in enumerate(pclouds):
        if not (p.dim() == 2 and p.shape[1] == 3 and p.shape[0] > 0):
            raise ValueError('%s: pclouds[%d] must be [P, 3] with P >= 1, got %s' % (who, n, tuple(p.shape)))
        if p.shape[0] != pclouds[0].shape[0]:
            raise ValueError('%s: pclouds[%d] has %d points and pclouds[0] has %d (one common P is expected: unequal sizes are refused)'
                             % (who, n, p.shape[0], pclouds[0].shape[0]))
        if p.dtype != torch.float32:
            raise ValueError('%s: pclouds[%d] must be float32, got %s' % (who, n, p.dtype))
    if len(pclouds) * pclouds[0].shape[0] * 3 >= 2 ** 31 - 1:
        raise ValueError('%s: pclouds with %d values are beyond int32 indexing' % (who, len(pclouds) * pclouds[0].shape[0] * 3))
    _check_devices(who, **{'pclouds[%d]' % n: p for n, p in enumerate(pclouds)})
    return list(pclouds)


# ------------------------------------------------------------------------------------------------ launches
def _fit(clouds, boxes, withangle, up, status):
    """es_cloud_fit on checked arguments -> (placed [O, P, 3], bounds [O, 6]); boxes None: the clouds are placed already.
    status: int32 [O] on the device, written by the launch."""
    O, P = clouds.shape[0], clouds.shape[1]
    clouds = clouds.contiguous()
    bounds = torch.empty(O, 6, dtype=torch.float32, device=clouds.device)
    placed = clouds
    if boxes is not None:
        boxes = _rows(boxes)
        placed = torch.empty_like(clouds)
    hip.check(hip.lib().es_cloud_fit(C.c_void_p(clouds.data_ptr()), O, P, hip.ptr(boxes), boxes.stride(0) if boxes is not None else 0,
                                     1 if withangle else 0, _UP[up], C.c_void_p(placed.data_ptr()) if boxes is not None else None,
                                     C.c_void_p(bounds.data_ptr()), C.c_void_p(status.data_ptr()), hip.current_stream()), 'es_cloud_fit')
    return placed, bounds


def _self_nn(placed):
    O, P = placed.shape[0], placed.shape[1]
    d11 = torch.empty(O, P, dtype=torch.float32, device=placed.device)
    hip.check(hip.lib().es_cloud_self_nn(C.c_void_p(placed.data_ptr()), O, P, C.c_void_p(d11.data_ptr()), hip.current_stream()),
              'es_cloud_self_nn')
    return d11


def _overlap(q, d11, c, cbounds, pairs, counts, status):
    hip.check(hip.lib().es_cloud_overlap(C.c_void_p(q.data_ptr()), q.shape[0], q.shape[1], C.c_void_p(d11.data_ptr()), C.c_void_p(c.data_ptr()),
                                         c.shape[0], c.shape[1], C.c_void_p(cbounds.data_ptr()), C.c_void_p(pairs.data_ptr()), pairs.shape[0],
                                         C.c_void_p(counts.data_ptr()), C.c_void_p(status.data_ptr()), hip.current_stream()),
              'es_cloud_overlap')


def _raise_on_fit_status(who, status):
    """status: the host copy of the fit's word per object"""
    flat = np.flatnonzero(status & 1)
    if len(flat):
        raise ValueError('%s: cloud %d has zero extent along an axis (the fit divides by it)' % (who, int(flat[0])))
    bad = np.flatnonzero(status & 2)
    if len(bad):
        raise ValueError('%s: cloud %d or its box holds a value that is not finite' % (who, int(bad[0])))


def _counts(clouds, boxes, pairs, up, fitted):
    """fit, self pass, pair pass on checked arguments -> one int32 buffer on the device: [pair status | fit status [O] | counts [K]]"""
    O, K = clouds.shape[0], pairs.shape[0]
    with torch.cuda.device(clouds.device):
        buf = torch.empty(1 + O + K, dtype=torch.int32, device=clouds.device)
        placed, bounds = _fit(clouds, None if fitted else boxes, True, up, buf[1:1 + O])
        d11 = _self_nn(placed)
        _overlap(placed, d11, placed, bounds, pairs.contiguous(), buf[1 + O:], buf[:1])
    return buf


def _raise_on_status(who, host, O):
    _raise_on_fit_status(who, host[1:1 + O])
    if host[0] & 1:
        raise ValueError('%s: a pair names a cloud outside [0, %d)' % (who, O))


# ------------------------------------------------------------------------------------------------ the calls
def fit_shapes_to_box(box, shape, withangle=True, up='z'):
    """The reference's function of this name (helpers/util.py) for one object (``box`` [7] or, with ``withangle=False``, [6]; ``shape``
    [P, 3]) or for O objects at once ([O, 7 | 6], [O, P, 3]) -> the placed cloud(s), float32 on the device, in the shape of ``shape``.
    A box row is (size x, y, z, centre x, y, z, angle in degrees).  ``up``: the axis the angle turns about, 'z' as the reference's
    ``get_rotation``, 'y' as its ``get_rotation_3dfront`` (the boxes of this package).  A cloud with zero extent along an axis, or a
    value that is not finite, raises a ValueError after the launch."""
    who = 'fit_shapes_to_box'
    _check_up(who, up)
    one = torch.is_tensor(shape) and shape.dim() == 2
    if one:
        shape = shape[None]
        if torch.is_tensor(box) and box.dim() == 1:
            box = box[None]
    _check_clouds(who, 'shape', shape)
    _check_boxes(who, box, shape.shape[0], bool(withangle))
    _check_devices(who, shape=shape, box=box)
    with torch.cuda.device(shape.device):
        status = torch.empty(shape.shape[0], dtype=torch.int32, device=shape.device)
        placed, _ = _fit(shape, box, bool(withangle), up, status)
        _raise_on_fit_status(who, status.cpu().numpy())
    return placed[0] if one else placed


def overlap_counts(clouds, boxes, pairs, up='z', fitted=False):
    """The whole-test-set call: ``clouds`` [O, P, 3], ``boxes`` [O, 7] (None is accepted with ``fitted=True``: the clouds are placed
    already and the fit is skipped), ``pairs`` int32 [K, 2] on the device -> int32 [K] on the device; ``out[k]`` counts the points of
    cloud ``pairs[k, 0]`` that have run into cloud ``pairs[k, 1]`` (the rule at the head of this module).  Both orders of a pair are
    accepted, and so is a pair of a cloud with itself (P, without duplicates).  A count depends on its two clouds and boxes alone: not
    on the run, the rest of the batch or the order of the list.  An index outside [0, O) raises a ValueError after the launch; nothing
    is read through it.  Scenes of a test set are concatenated with node offsets (``eligible_pairs(..., offsets=)``)."""
    who = 'overlap_counts'
    _check_up(who, up)
    _check_clouds(who, 'clouds', clouds)
    O = clouds.shape[0]
    if not fitted or boxes is not None:
        _check_boxes(who, boxes, O, True)
    if not torch.is_tensor(pairs):
        raise ValueError('%s: pairs must be a tensor [K, 2], got %s' % (who, type(pairs).__name__))
    if pairs.dtype != torch.int32:
        raise ValueError('%s: pairs must be int32, got %s' % (who, pairs.dtype))
    if not (pairs.dim() == 2 and pairs.shape[1] == 2):
        raise ValueError('%s: pairs must be [K, 2], got %s' % (who, tuple(pairs.shape)))
    if pairs.shape[0] >= 2 ** 31 - 1 - O:
        raise ValueError('%s: %d pairs are beyond int32 indexing' % (who, pairs.shape[0]))
    _check_devices(who, clouds=clouds, boxes=None if fitted else boxes, pairs=pairs)
    K = pairs.shape[0]
    if K == 0:
        return torch.empty(0, dtype=torch.int32, device=clouds.device)
    buf = _counts(clouds, boxes, pairs, up, fitted)
    _raise_on_status(who, buf[:1 + O].cpu().numpy(), O)
    return buf[1 + O:]


def pointcloud_overlap_pair(pc1, pc2):
    """The reference's function of this name for two placed clouds [P1, 3] and [P2, 3] (P1 and P2 may differ) -> a Python int: the
    points of ``pc1`` whose nearest point of ``pc2`` is strictly nearer than their nearest other point of ``pc1``.  On an exact tie of
    the two distances the own cloud wins (the reference follows its kd-tree's visiting order there)."""
    who = 'pointcloud_overlap_pair'
    for name, x in (('pc1', pc1), ('pc2', pc2)):
        if not (torch.is_tensor(x) and x.dim() == 2):
            raise ValueError('%s: %s must be a tensor [P, 3]' % (who, name))
    q, c = pc1[None], pc2[None]
    _check_clouds(who, 'pc1', q)
    _check_clouds(who, 'pc2', c)
    _check_devices(who, pc1=pc1, pc2=pc2)
    with torch.cuda.device(q.device):
        buf = torch.empty(4, dtype=torch.int32, device=q.device)
        q, qb = _fit(q, None, True, 'z', buf[1:2])
        c, cb = _fit(c, None, True, 'z', buf[2:3])
        pairs = torch.zeros(1, 2, dtype=torch.int32, device=q.device)
        _overlap(q, _self_nn(q), c, cb, pairs, buf[3:], buf[:1])
        host = buf.cpu().numpy()
    _raise_on_fit_status(who, host[1:3])
    return int(host[3])


def eligible_pairs(objs, triples, vocab, offsets=None):
    """The pairs (i, j), i < j in lexicographic order, that the reference's ``pointcloud_overlap`` judges: int32 [K, 2] on the host
    (``.cuda()`` makes it the ``pairs`` of ``overlap_counts``).  Host only.  ``objs``: the class id of each node; ``triples`` [T, 3]
    rows (s, p, o); ``vocab``: ``object_idx_to_name`` and ``pred_idx_to_name``, each name read up to its first newline.  A pair is left
    out when either object is one of ``STRUCTURAL``, or when the predicate stated for (i, j) or for (j, i) is one of ``TOUCHING``; of two
    triples with the same (s, o) the later one decides, as in the reference's ``dict(zip(...))``.  ``offsets`` [S + 1]: the node ranges of
    S scenes concatenated with node offsets; pairs never cross scenes and carry global indices."""
    who = 'eligible_pairs'
    onames = vocab.get('object_idx_to_name') if isinstance(vocab, dict) else None
    pnames = vocab.get('pred_idx_to_name') if isinstance(vocab, dict) else None
    for key, names in (('object_idx_to_name', onames), ('pred_idx_to_name', pnames)):
        if not (isinstance(names, (list, tuple)) and len(names) > 0 and all(isinstance(n, str) for n in names)):
            raise ValueError("%s: vocab['%s'] must be a non-empty list of names" % (who, key))
    objs = np.asarray(objs.cpu() if torch.is_tensor(objs) else objs)
    triples = np.asarray(triples.cpu() if torch.is_tensor(triples) else triples)
    if objs.size == 0:
        objs = np.zeros(0, np.int64)
    if not (objs.ndim == 1 and objs.dtype.kind in 'iu'):
        raise ValueError('%s: objs must be integers [O], got %s %s' % (who, objs.dtype, objs.shape))
    if triples.size == 0:
        triples = np.zeros((0, 3), np.int64)
    if not (triples.ndim == 2 and triples.shape[1] == 3 and triples.dtype.kind in 'iu'):
        raise ValueError('%s: triples must be integers [T, 3], got %s %s' % (who, triples.dtype, triples.shape))
    O = len(objs)
    if O and (objs.min() < 0 or objs.max() >= len(onames)):
        raise ValueError('%s: objs names a class outside [0, %d)' % (who, len(onames)))
    if len(triples) and (triples[:, 1].min() < 0 or triples[:, 1].max() >= len(pnames)):
        raise ValueError('%s: a triple names a predicate outside [0, %d)' % (who, len(pnames)))
    if offsets is None:
        offsets = [0, O]
    offsets = [int(v) for v in (offsets.tolist() if hasattr(offsets, 'tolist') else offsets)]
    if not (len(offsets) >= 2 and offsets[0] == 0 and offsets[-1] == O and all(a <= b for a, b in zip(offsets, offsets[1:]))):
        raise ValueError('%s: offsets must rise from 0 to O = %d, got %s' % (who, O, offsets))
    structural = [onames[c].split('\n')[0] in STRUCTURAL for c in objs.tolist()]
    touching = [n.split('\n')[0] in TOUCHING for n in pnames]
    pair2pred = {(s, o): p for s, p, o in triples.tolist()}
    out = []
    for lo, hi in zip(offsets, offsets[1:]):
        for i in range(lo, hi - 1):
            for j in range(i + 1, hi):
                if structural[i] or structural[j]:
                    continue
                if (i, j) in pair2pred and touching[pair2pred[(i, j)]]:
                    continue
                if (j, i) in pair2pred and touching[pair2pred[(j, i)]]:
                    continue
                out.append((i, j))
    return torch.from_numpy(np.array(out, np.int32).reshape(-1, 2))


def pointcloud_overlap(pclouds, objs, boxes, angles, triples, vocab, overlap_metric, up='z'):
    """The reference's function of this name: appends one count per eligible pair (``eligible_pairs``), first cloud i against second
    cloud j, to ``overlap_metric`` in the reference's order and returns the list.  ``pclouds``: [O, P, 3] or a list of O tensors [P, 3]
    with one common P (unequal sizes are refused); ``boxes`` [O, 6] and ``angles`` [O] or [O, 1] (degrees) are joined as the reference
    joins them; ``up='z'`` is the reference's rotation, ``up='y'`` the convention of this package's boxes.  One fit launch, one self pass,
    one pair pass and one copy to the host; a scene without an eligible pair returns the list untouched without a launch."""
    who = 'pointcloud_overlap'
    _check_up(who, up)
    if not isinstance(overlap_metric, list):
        raise ValueError('%s: overlap_metric must be a list, got %s' % (who, type(overlap_metric).__name__))
    clouds = _check_cloud_list(who, pclouds)
    O = len(clouds)
    if not (torch.is_tensor(boxes) and boxes.dim() == 2 and boxes.shape[1] >= 6 and boxes.shape[0] == O):
        raise ValueError('%s: boxes must be a tensor [%d, 6], one row per cloud' % (who, O))
    if not (torch.is_tensor(angles) and angles.numel() == O):
        raise ValueError('%s: angles must be a tensor with one entry per cloud (%d)' % (who, O))
    if len(objs) != O:
        raise ValueError('%s: %d objs for %d clouds' % (who, len(objs), O))
    pairs = eligible_pairs(objs, triples, vocab)
    _check_devices(who, pclouds=clouds[0], boxes=boxes, angles=angles)
    if len(pairs) == 0:
        return overlap_metric
    if isinstance(clouds, list):
        clouds = torch.stack(clouds)
    boxes7 = torch.cat([boxes[:, :6].float(), angles.reshape(-1, 1).float()], 1)                       # the reference's own join
    buf = _counts(clouds, boxes7, pairs.to(clouds.device), up, False)
    host = buf.cpu().numpy()
    _raise_on_status(who, host, O)
    overlap_metric.extend(int(v) for v in host[1 + O:])
    return overlap_metric
