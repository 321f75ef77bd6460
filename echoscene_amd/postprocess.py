"""Device-side versions of the two box helpers the caller applies right after the path
(scripts/eval_3dfront.py:283-284; reference helpers/util.py:542-568) -- SURVEY.md section 8(f) rank 3.
Same names and semantics (``descale_box_params`` writes into its argument and returns it)."""
import ctypes as C
import numpy as np
import torch

from . import hip


def descale_box_params(normed_box_params, file=None, angle=False, stats=None):
    """[-1,1] -> dataset units for sizes (cols 0:3) and translations (cols 3:6), in place on a CUDA tensor; ``angle=True``: also
    column 6, a normalised angle, to [stats[12], stats[13]] (helpers/util.py:553-555)."""
    assert file is not None or stats is not None
    ncol = 7 if angle else 6
    st = np.loadtxt(file) if stats is None else np.asarray(stats)
    if st.size < (14 if angle else 12):
        raise ValueError('descale_box_params: %d statistics given, %d needed%s' % (st.size, 14 if angle else 12, ' (angle=True reads entries 12, 13)' if angle else ''))
    x = normed_box_params
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] >= ncol and x.stride(1) == 1):
        raise ValueError('descale_box_params: expects a float32 CUDA tensor [O, >=%d]' % ncol)
    std = torch.tensor(st, dtype=torch.float32, device=x.device)
    hip.check(hip.lib().es_box_descale(C.c_void_p(x.data_ptr()), x.stride(0), ncol, C.c_void_p(std.data_ptr()), x.shape[0],
                                       hip.current_stream()), 'es_box_descale')
    return x


def scale_box_params(box_params, file=None, angle=False, stats=None):
    """Dataset units -> [-1,1] for sizes (cols 0:3) and translations (cols 3:6) of a float32 CUDA tensor [O, >=6], in place and
    returned; ``angle=True``: also column 6, a metric angle, from [stats[12], stats[13]] (helpers/util.py:516-532, which handles one box
    at a time).  The inverse of ``descale_box_params``: a box of a dataset scene or of a de-normalised result becomes a row that
    ``keep_boxes`` takes.  Evaluated in double on the float64 statistics and rounded once (es_box_prescale)."""
    assert file is not None or stats is not None
    ncol = 7 if angle else 6
    st = np.loadtxt(file) if stats is None else np.asarray(stats, dtype=np.float64)
    if st.size != 14:
        raise NotImplementedError('scale_box_params: %d statistics given, 14 needed (helpers/util.py:519-522)' % st.size)
    x = box_params
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] >= ncol and x.stride(1) == 1):
        raise ValueError('scale_box_params: expects a float32 CUDA tensor [O, >=%d]' % ncol)
    std = torch.tensor(st.reshape(-1), dtype=torch.float64, device=x.device)
    hip.check(hip.lib().es_box_prescale(C.c_void_p(x.data_ptr()), x.stride(0), ncol, None, C.c_void_p(std.data_ptr()),
                                        C.c_void_p(x.data_ptr()), x.stride(0), None, x.shape[0], hip.current_stream()), 'es_box_prescale')
    return x


def preprocess_angle2sincos(angle):
    """[O,1] angle in radians -> [O,2] (sin, cos) (helpers/util.py:534-540); the inverse of ``postprocess_sincos2arctan``."""
    if not (angle.is_cuda and angle.dtype == torch.float32 and angle.dim() == 2 and angle.shape[1] == 1):
        raise ValueError('preprocess_angle2sincos: expects a float32 CUDA tensor [O, 1]')
    a = angle.contiguous()
    out = torch.empty(a.shape[0], 2, dtype=torch.float32, device=a.device)
    hip.check(hip.lib().es_box_prescale(None, 0, 0, C.c_void_p(a.data_ptr()), None, None, 0, C.c_void_p(out.data_ptr()), a.shape[0],
                                        hip.current_stream()), 'es_box_prescale')
    return out


def postprocess_sincos2arctan(sincos):
    """[O,2] (sin, cos) -> [O,1] angle in radians."""
    B, N = sincos.shape
    assert N == 2
    s = sincos.contiguous()
    out = torch.empty(B, 1, dtype=torch.float32, device=s.device)
    hip.check(hip.lib().es_box_postprocess(None, 0, C.c_void_p(s.data_ptr()), C.c_void_p(out.data_ptr()), None, B, 1.0,
                                           hip.current_stream()), 'es_box_postprocess')
    return out


def range_bounds(ranges, n):
    """The integer bounds of get_partial_shape (diffusion_shape/diff_utils/demo_util.py:183-201, :232-239) for a grid of ``n`` cells
    per axis: ``ranges`` = K dicts {'x': (a, b), 'y': (a, b), 'z': (a, b)} in [-1, 1] (the reference's xyz_dict; one dict is K = 1) ->
    int32 [K, 6] = (st, ed) of 'x', 'y', 'z' -- dims 2, 3 and 4 of a [B, 1, n, n, n] tensor.  The reference's rule in Python floats, as
    it is written there: each end clamped to [-1, 1], then int((v - (-1)) / 2 * n).  A voxel is inside when st <= index < ed on all
    three axes; st >= ed on any axis selects nothing.  Host only."""
    if isinstance(ranges, dict):
        ranges = [ranges]
    out = np.zeros((len(ranges), 6), np.int32)
    for k, r in enumerate(ranges):
        if not isinstance(r, dict) or set(r) != {'x', 'y', 'z'}:
            raise ValueError("range_bounds: entry %d must be a dict with the keys 'x', 'y', 'z' (each a (min, max) pair), got %r" % (k, r))
        for a, key in enumerate(('x', 'y', 'z')):
            lo, hi = r[key]
            lo, hi = max(-1, lo), min(1, hi)
            out[k, 2 * a] = int((lo - (-1)) / 2 * n)
            out[k, 2 * a + 1] = int((hi - (-1)) / 2 * n)
    return out


def latent_range_mask(ranges, zdims=(16, 16, 16), device=None):
    """``z_mask`` of get_partial_shape (demo_util.py:229-252) for K ranges: f32 [K, 1, *zdims] on ``device``, 1 on the latent voxels
    inside the range -- what ``complete_masks=`` of the scene calls and a per-voxel ``mask=`` of ShapeDenoiser.sample take.  The
    reference assumes a cubic grid; so does this (es_range_mask)."""
    zdims = tuple(int(d) for d in zdims)
    if len(zdims) != 3 or len(set(zdims)) != 1:
        raise ValueError('latent_range_mask: zdims must be a cubic grid (n, n, n), got %r' % (zdims,))
    device = torch.device('cuda') if device is None else torch.device(device)
    b = torch.from_numpy(range_bounds(ranges, zdims[0])).to(device)
    K = b.shape[0]
    out = torch.empty(K, 1, *zdims, dtype=torch.float32, device=device)
    if K:
        hip.check(hip.lib().es_range_mask(C.c_void_p(b.data_ptr()), K, zdims[0], zdims[1], zdims[2], C.c_void_p(out.data_ptr()),
                                          hip.current_stream()), 'es_range_mask')
    return out


def partial_shape(sdf, ranges, fill=0.2, zdims=(16, 16, 16)):
    """get_partial_shape (demo_util.py:172-254) for SDF grids [K, 1, n, n, n] on the device, one range per grid (``ranges`` as
    range_bounds): a dict of ``shape_part`` (the SDF inside the range, ``fill`` -- the truncation value -- outside), ``shape_missing``
    (the complement), ``shape_mask`` (bool [K, 1, n, n, n]) and ``z_mask`` (latent_range_mask at ``zdims``), all on the device.
    ``shape_part`` is what a caller with a truly partial scan hands to ``complete_sdfs=``: the encoder then sees the truncation value,
    not the shape, outside the range."""
    x = sdf
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and x.shape[1] == 1
            and x.shape[2] == x.shape[3] == x.shape[4]):
        raise ValueError('partial_shape: expects a float32 CUDA tensor [K, 1, n, n, n]')
    x = x.contiguous()
    K, n = x.shape[0], x.shape[2]
    bounds = range_bounds(ranges, n)
    if bounds.shape[0] != K:
        raise ValueError('partial_shape: %d ranges for %d SDFs (one range per grid)' % (bounds.shape[0], K))
    b = torch.from_numpy(bounds).to(x.device)
    part, missing = torch.empty_like(x), torch.empty_like(x)
    smask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if K:
        hip.check(hip.lib().es_partial_shape(C.c_void_p(x.data_ptr()), C.c_void_p(b.data_ptr()), K, n, float(fill),
                                             C.c_void_p(part.data_ptr()), C.c_void_p(missing.data_ptr()), C.c_void_p(smask.data_ptr()),
                                             hip.current_stream()), 'es_partial_shape')
    return {'shape_part': part, 'shape_missing': missing, 'shape_mask': smask.bool(),
            'z_mask': latent_range_mask(ranges, zdims, x.device)}


_MC_TABLE = {}


def _mc_table(device):
    from .mc_tables import tri_table
    key = str(device)
    if key not in _MC_TABLE:
        _MC_TABLE[key] = torch.from_numpy(tri_table().copy()).to(device)
    return _MC_TABLE[key]


def marching_cubes_batch(sdf, level=0.02):
    """SDF grids -> indexed triangle meshes on the device (csrc/es_mc.hip).

    ``sdf``: float32 CUDA tensor [O, n, n, n] (or [O, 1, n, n, n], the layout ``rel2shape`` returns).  Returns a list of
    (verts f32 [V,3] in grid-index units, faces int64 [T,3]) per object, CUDA tensors -- the values
    ``mcubes.marching_cubes(sdf[i, 0].cpu().numpy(), level)`` produces in the reference (util_3d.py:214-217) for the VERTEX SET
    (one vertex per sign-changing grid edge, same interpolation), up to their order.  The FACES follow this package's own case
    table (mc_tables.py): the diagonals inside a cell AND, on ambiguous-face cases, the loop structure / triangle count differ
    from PyMCubes' classic table (44 case / complement pairs) -- face counts and topology can differ there; meshes are
    watertight either way."""
    if sdf.dim() == 5:
        assert sdf.shape[1] == 1
        sdf = sdf[:, 0]
    if not (sdf.is_cuda and sdf.dim() == 4 and sdf.shape[1] == sdf.shape[2] == sdf.shape[3]):
        raise ValueError('marching_cubes_batch: expects a CUDA tensor [O, n, n, n]')
    sdf = sdf.contiguous().float()
    O, n = sdf.shape[0], sdf.shape[1]
    dev = sdf.device
    L = hip.lib()
    tab = _mc_table(dev)
    ws = torch.empty(L.es_marching_cubes_workspace(O, n), dtype=torch.uint8, device=dev)
    counts = torch.empty(2 * O, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    hip.check(L.es_marching_cubes_count(p(sdf), O, n, float(level), p(tab), p(ws), p(counts), hip.current_stream()),
              'es_marching_cubes_count')
    c = counts.cpu().view(O, 2).long()                     # the one host round trip: output sizes are data dependent
    vofs = torch.cat([torch.zeros(1, dtype=torch.long), c[:, 0].cumsum(0)])
    tofs = torch.cat([torch.zeros(1, dtype=torch.long), c[:, 1].cumsum(0)])
    verts = torch.empty(max(int(vofs[-1]), 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(int(tofs[-1]), 1), 3, dtype=torch.int32, device=dev)
    vo, to = vofs[:-1].contiguous().to(dev), tofs[:-1].contiguous().to(dev)
    hip.check(L.es_marching_cubes_emit(p(sdf), O, n, float(level), p(tab), p(ws), p(vo), p(to), p(verts), p(faces),
                                       hip.current_stream()), 'es_marching_cubes_emit')
    return [(verts[int(vofs[o]):int(vofs[o + 1])], faces[int(tofs[o]):int(tofs[o + 1])].long()) for o in range(O)]


def marching_cubes(sdf_i, level):
    """Same call shape as ``mcubes.marching_cubes(volume, isovalue)`` for one [n,n,n] CUDA grid -> (verts, faces)."""
    return marching_cubes_batch(sdf_i[None], level)[0]


def sdf_to_mesh(sdf, level=0.02, render_all=False):
    """util_3d.sdf_to_mesh (model/diff_utils/util_3d.py:194-236) up to the pytorch3d container: per-object vertex lists
    normalised like the reference (``verts / n_cell - 0.5``) and int64 faces, at most 16 objects unless ``render_all``."""
    bs, n_cell = sdf.shape[0], sdf.shape[-1]
    k = bs if render_all else min(bs, 16)
    meshes = marching_cubes_batch(sdf[:k], level)
    return [v / n_cell - 0.5 for v, _ in meshes], [f for _, f in meshes]


def mesh_to_sdf(meshes, n=64, trunc=0.2, fit=0.9, return_transform=False):
    """Triangle meshes -> truncated SDF grids on the device (csrc/es_mesh_sdf.hip): the inverse of ``sdf_to_mesh``.

    ``meshes``: a list of (verts [V,3] floating point, faces [T,3] integer with vertex ids local to the mesh) pairs of CUDA tensors --
    what ``marching_cubes_batch`` returns -- or one such pair.  Returns float32 [K, 1, n, n, n], exactly what ``keep_sdfs=`` and
    ``complete_sdfs=`` of the scene calls take: voxel (i, j, k) is the point (i/n - 0.5, j/n - 0.5, k/n - 0.5) (the normalisation of
    ``sdf_to_mesh``: ``verts / n_cell - 0.5``), array axes are x, y, z, the value is the exact distance to the nearest triangle,
    negative inside, clamped to [-trunc, trunc] (the reference clamps its grids to +-0.2, dataset/threedfront_dataset.py:313-317).
    Inside is where the generalized winding number exceeds 0.5: the sign of a closed mesh, and a usable one for meshes with holes or
    self-intersections.  Triangles of zero area are ignored.

    ``fit=s`` (0 < s <= 1) centres each mesh on the bounding box of its vertices and scales it so that the longest side of the box is
    ``s``, on the device.  The default 0.9 leaves 0.05 of margin (3.2 voxels at 64^3), enough for the 0.02 iso-level of
    ``sdf_to_mesh``; it is THIS PACKAGE'S CHOICE, not the dataset's normalisation: the reference reads grids that a tool outside it
    wrote, and fits generated meshes to their layout boxes afterwards anyway.  ``fit=None`` takes the coordinates as they are.
    ``return_transform=True`` also returns float32 [K, 4]: centre x, y, z and scale of each mesh, fitted = (v - centre) * scale.

    Every refusal of the arguments is a ValueError raised before any device work; a face index outside its mesh is caught on the
    device (never dereferenced) and raised as a ValueError after the call."""
    if isinstance(meshes, tuple) and len(meshes) == 2 and torch.is_tensor(meshes[0]):
        meshes = [meshes]
    if not isinstance(meshes, (list, tuple)) or len(meshes) == 0:
        raise ValueError('mesh_to_sdf: expects a non-empty list of (verts, faces) pairs')
    if not isinstance(n, (int, np.integer)) or isinstance(n, bool) or n < 2:
        raise ValueError('mesh_to_sdf: n must be an integer >= 2, got %r' % (n,))
    n = int(n)
    if not trunc > 0:
        raise ValueError('mesh_to_sdf: trunc must be positive, got %r' % (trunc,))
    if fit is not None and not 0 < fit <= 1:
        raise ValueError('mesh_to_sdf: fit must be in (0, 1] (or None: coordinates as given), got %r' % (fit,))
    K = len(meshes)
    if K * n ** 3 >= 2 ** 31:
        raise ValueError('mesh_to_sdf: %d grids of %d^3 are beyond int32 indexing' % (K, n))
    dev = None
    for k, mesh in enumerate(meshes):
        if not (isinstance(mesh, (list, tuple)) and len(mesh) == 2 and torch.is_tensor(mesh[0]) and torch.is_tensor(mesh[1])):
            raise ValueError('mesh_to_sdf: mesh %d is not a (verts, faces) pair of tensors' % k)
        v, f = mesh
        if not (v.dim() == 2 and v.shape[1] == 3 and v.is_floating_point()):
            raise ValueError('mesh_to_sdf: verts of mesh %d must be a floating-point tensor [V, 3], got %s %s' % (k, v.dtype, tuple(v.shape)))
        if not (f.dim() == 2 and f.shape[1] == 3 and f.dtype in (torch.int32, torch.int64)):
            raise ValueError('mesh_to_sdf: faces of mesh %d must be an int32 / int64 tensor [T, 3], got %s %s' % (k, f.dtype, tuple(f.shape)))
        if f.shape[0] == 0 or v.shape[0] == 0:
            raise ValueError('mesh_to_sdf: mesh %d has no %s' % (k, 'faces' if f.shape[0] == 0 else 'vertices'))
    for k, (v, f) in enumerate(meshes):
        if not (v.is_cuda and f.is_cuda):
            raise ValueError('mesh_to_sdf: mesh %d is not on the device (CUDA tensors expected)' % k)
        dev = v.device if dev is None else dev
        if v.device != dev or f.device != dev:
            raise ValueError('mesh_to_sdf: mesh %d is on %s / %s, the first mesh on %s' % (k, v.device, f.device, dev))
    vofs = np.cumsum([0] + [int(m[0].shape[0]) for m in meshes])
    tofs = np.cumsum([0] + [int(m[1].shape[0]) for m in meshes])
    L = hip.lib()
    with torch.cuda.device(dev):
        verts = torch.cat([m[0].float() for m in meshes]).contiguous()
        # (an int64 id beyond int32 stays out of range after the cast)
        faces = torch.cat([m[1].clamp(-1, 2 ** 31 - 1).int() if m[1].dtype == torch.int64 else m[1] for m in meshes]).contiguous()
        vo, to = torch.from_numpy(vofs).to(dev), torch.from_numpy(tofs).to(dev)
        ws = torch.empty(L.es_mesh_sdf_workspace(K, int(tofs[-1])), dtype=torch.uint8, device=dev)
        bad = torch.empty(K, dtype=torch.int32, device=dev)
        tf = torch.empty(K, 4, dtype=torch.float32, device=dev)
        out = torch.empty(K, 1, n, n, n, dtype=torch.float32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        hip.check(L.es_mesh_sdf(p(verts), p(faces), p(vo), p(to), K, int(vofs[-1]), int(tofs[-1]), n, float(trunc),
                                0.0 if fit is None else float(fit), p(ws), p(bad), p(tf), p(out), hip.current_stream()), 'es_mesh_sdf')
        flagged = bad.cpu().nonzero().flatten().tolist()
    if flagged:
        raise ValueError('mesh_to_sdf: meshes %s have a face index outside [0, V)' % flagged)
    return (out, tf) if return_transform else out
