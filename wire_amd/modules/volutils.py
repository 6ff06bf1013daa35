"""Volume helpers on the hot path's contract (reference modules/volutils.py).

What the occupancy training / evaluation loop touches (wire_occupancy.py:160-172), the IoU metric, and what its last
lines do (wire_occupancy.py:198-201): ``march_and_save`` and ``export_mesh``, the volume's iso-surface written as a
mesh file.  The counts of the IoU are reduced on the device (wire_eval_metric mode 1): no host pass over the 134 M
voxels of a 512^3 volume.  The mesh is extracted on the device too (functional.iso_surface: marching tetrahedra on
the Kuhn split, csrc/wire_iso.hip) -- the reference calls PyMCubes there, so the triangles differ from the reference's
while the surface they tile is the same level set; and ``smoothen`` blurs the binarised volume with a Gaussian
(wire_gauss3_blur), NOT PyMCubes' ``smooth``, which blurs a signed distance transform and cannot be reproduced or
compared here.  Only the file writers (.obj, binary .ply, COLLADA .dae) run on the host.  The open3d point-cloud
helpers, noise models and SSIM helpers of the reference's module stay out of scope.
"""
from __future__ import annotations

import datetime
import os

import numpy as np
import torch

from .. import _lib
from .. import functional as _F


def get_I_and_U(preds, gt, thres=None):
    """Intersection and union counts (modules/volutils.py:78-91).  As in the reference, ``preds`` is binarised
    IN PLACE when ``thres`` is given -- the caller's tensor afterwards holds 0 / 1 (wire_occupancy.py keeps that
    binarised volume as ``best_img``).  CUDA float32 tensors take the device reduction; numpy arrays the
    reference's own numpy expression."""
    if isinstance(preds, np.ndarray):
        if thres is not None:
            preds[preds < thres] = 0.0
            preds[preds >= thres] = 1.0
        return np.logical_and(preds, gt).sum(), np.logical_or(preds, gt).sum()
    if not preds.is_cuda:
        raise _lib.WireHipError("get_I_and_U: tensors must be on the MI355X ('cuda'); wire_amd has no CPU path")
    L = _lib.lib()
    p = preds.detach()
    g = gt.detach().to(p.device, torch.float32).contiguous()
    if thres is not None:
        p.masked_fill_(p < thres, 0.0)
        p.masked_fill_(p >= thres, 1.0)
    # without a threshold the reference's logical_and / logical_or test for non-zero (either sign)
    flat = p.to(torch.float32).contiguous() if thres is not None else (p != 0).to(torch.float32).contiguous()
    # exact integer counts, as the reference's logical_and(...).sum(): the device reduction accumulates in fp32, which
    # holds every integer up to 2^24, so the volume goes in slabs of at most 2^24 voxels (a 512^3 volume has 2^27) whose
    # counts are converted to int64 before they are added up -- all on the device, no host sync
    out = torch.empty(2, dtype=torch.float32, device=p.device)
    partial = torch.empty(4096, dtype=torch.float32, device=p.device)
    flat, g = flat.reshape(-1), g.reshape(-1)
    inter = torch.zeros((), dtype=torch.int64, device=p.device)
    union = torch.zeros((), dtype=torch.int64, device=p.device)
    stream = torch.cuda.current_stream(p.device).cuda_stream
    for b in range(0, flat.numel(), 1 << 24):
        n = min(1 << 24, flat.numel() - b)
        # the volume now holds 0 / 1: counting "pred >= 0.5" counts its ones
        _lib.check(L.wire_eval_metric(stream, 1, flat.data_ptr() + 4 * b, g.data_ptr() + 4 * b, n, 0.5, out.data_ptr(),
                                      partial.data_ptr()), "wire_eval_metric")
        cnt = out.to(torch.int64)
        inter = inter + cnt[0]
        union = union + cnt[1]
    return inter, union


def get_IoU(preds, gt, thres=None):
    """modules/volutils.py:74-76."""
    intersection, union = get_I_and_U(preds, gt, thres)
    return intersection / union


def get_IoU_batch(preds, gt, thres=None, maxpoints=pow(2, 24)):
    """modules/volutils.py:54-71: IoU accumulated over slabs of ``maxpoints`` voxels."""
    preds, gt = preds.flatten(), gt.flatten()
    inter, union = [], []
    for b in range(0, preds.numel(), maxpoints):
        i, u = get_I_and_U(preds[b:b + maxpoints], gt[b:b + maxpoints], thres)
        inter.append(i)
        union.append(u)
    return sum(inter) / sum(union)


def query_occupancy(coords, cube_res, model, batchsize, occupancy=None):
    """The dense query of ``export_mesh`` (modules/volutils.py:113-133): ``model`` is evaluated on ``coords``
    ((cube_res^3, 3), host or device) in batches of ``batchsize``, ``torch.sigmoid`` of the output fills a
    (cube_res, cube_res, cube_res) float32 numpy cube -- what the reference then hands to ``mcubes.marching_cubes``
    and ``export_mesh`` here to ``functional.iso_surface``.  The network forward is the fused HIP path; the sigmoid is
    wire_sigmoid_inplace."""
    n = cube_res ** 3
    if occupancy is None:
        occupancy = np.zeros((n, 1), dtype=np.float32)
    else:
        occupancy[...] = 0
        occupancy = occupancy.reshape(-1, 1)
    L = _lib.lib()
    with torch.no_grad():
        for b in range(0, n, batchsize):
            b2 = min(b + batchsize, n)
            sub = coords[b:b2, :].cuda()
            y = model(sub).contiguous()
            _lib.check(L.wire_sigmoid_inplace(torch.cuda.current_stream(y.device).cuda_stream, y.data_ptr(), y.numel()),
                       "wire_sigmoid_inplace")
            occupancy[b:b2, :] = y.cpu().numpy()
    return occupancy.reshape(cube_res, cube_res, cube_res)


# ---------------------------------------------------------------------------
# mesh files (host side): Wavefront .obj, binary little-endian .ply, COLLADA 1.4.1 .dae
# ---------------------------------------------------------------------------
def _write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.write("# wire_amd iso-surface: %d vertices, %d faces\n" % (len(v), len(f)))
        np.savetxt(fh, v, fmt="v %.9g %.9g %.9g")
        np.savetxt(fh, f + 1, fmt="f %d %d %d")


def _write_ply(path, v, f):
    rec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    rec["n"], rec["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\ncomment wire_amd iso-surface\nelement vertex %d\n"
                  "property float x\nproperty float y\nproperty float z\nelement face %d\n"
                  "property list uchar int vertex_indices\nend_header\n" % (len(v), len(f))).encode("ascii"))
        fh.write(v.astype("<f4").tobytes())
        fh.write(rec.tobytes())


def _write_dae(path, v, f):
    """A minimal COLLADA 1.4.1 document: one geometry with one float_array and one <triangles>, instantiated by one node
    of one visual scene."""
    now = datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ")
    with open(path, "w") as fh:
        fh.write('<?xml version="1.0" encoding="utf-8"?>\n'
                 '<COLLADA xmlns="http://www.collada.org/2005/11/COLLADASchema" version="1.4.1">\n'
                 '  <asset>\n    <contributor><authoring_tool>wire_amd</authoring_tool></contributor>\n'
                 f'    <created>{now}</created>\n    <modified>{now}</modified>\n'
                 '    <unit name="meter" meter="1"/>\n    <up_axis>Y_UP</up_axis>\n  </asset>\n'
                 '  <library_geometries>\n    <geometry id="mesh" name="mesh">\n      <mesh>\n'
                 '        <source id="mesh-positions">\n'
                 f'          <float_array id="mesh-positions-array" count="{v.size}">')
        fh.write(" ".join("%.9g" % x for x in v.reshape(-1).tolist()))
        fh.write('</float_array>\n          <technique_common>\n'
                 f'            <accessor source="#mesh-positions-array" count="{len(v)}" stride="3">\n'
                 '              <param name="X" type="float"/>\n              <param name="Y" type="float"/>\n'
                 '              <param name="Z" type="float"/>\n            </accessor>\n'
                 '          </technique_common>\n        </source>\n'
                 '        <vertices id="mesh-vertices">\n'
                 '          <input semantic="POSITION" source="#mesh-positions"/>\n        </vertices>\n'
                 f'        <triangles count="{len(f)}">\n'
                 '          <input semantic="VERTEX" source="#mesh-vertices" offset="0"/>\n          <p>')
        fh.write(" ".join("%d" % i for i in f.reshape(-1).tolist()))
        fh.write('</p>\n        </triangles>\n      </mesh>\n    </geometry>\n  </library_geometries>\n'
                 '  <library_visual_scenes>\n    <visual_scene id="scene" name="scene">\n'
                 '      <node id="mesh-node" name="mesh" type="NODE">\n        <instance_geometry url="#mesh"/>\n'
                 '      </node>\n    </visual_scene>\n  </library_visual_scenes>\n'
                 '  <scene>\n    <instance_visual_scene url="#scene"/>\n  </scene>\n</COLLADA>\n')


_WRITERS = {".obj": _write_obj, ".ply": _write_ply, ".dae": _write_dae}


def save_mesh(vertices, faces, savename):
    """Write a triangle mesh (``vertices`` [V, 3], ``faces`` [F, 3]; tensors or arrays) in the format ``savename``'s
    extension names: ``.obj``, ``.ply`` (binary little-endian) or ``.dae`` (COLLADA 1.4.1, what the reference's drivers
    save).  Another extension is a ValueError."""
    ext = os.path.splitext(str(savename))[1].lower()
    if ext not in _WRITERS:
        raise ValueError(f"save_mesh: {savename!r}: the extension must be one of {sorted(_WRITERS)}")
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    v = np.ascontiguousarray(to_np(vertices), dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(to_np(faces), dtype=np.int32).reshape(-1, 3)
    _WRITERS[ext](str(savename), v, f)


def _device_volume(occupancy, what):
    if isinstance(occupancy, np.ndarray):
        if occupancy.ndim != 3:
            raise ValueError(f"{what} expects a rank-3 (H, W, T) volume")
        return torch.from_numpy(np.ascontiguousarray(occupancy, dtype=np.float32)).cuda()
    if not isinstance(occupancy, torch.Tensor) or occupancy.dim() != 3:
        raise ValueError(f"{what} expects a rank-3 (H, W, T) volume")
    if not occupancy.is_cuda:
        raise _lib.WireHipError(f"{what}: a tensor must be on the MI355X ('cuda'); pass a numpy array from the host")
    return occupancy.detach().to(torch.float32).contiguous()


def march(occupancy, mcubes_thres, smoothen=False):
    """The mesh that ``march_and_save`` writes: ``(vertices [V, 3] float32, faces [F, 3] int32)`` on the device."""
    vol = _device_volume(occupancy, "march_and_save")
    thres = float(mcubes_thres)
    if smoothen:
        # the caller's volume is left as it is (the reference copies it too): 1 where >= thres, 0 elsewhere (NaN too),
        # minus one half, blurred with sigma = 1, cut at 0
        vol = _F.gauss3_blur((vol >= thres).to(torch.float32) - 0.5, 1.0)
        thres = 0.0
    return _F.iso_surface(vol, thres)


def march_and_save(occupancy, mcubes_thres, savename, smoothen=False):
    """modules/volutils.py:413-438 with the reference's signature: the iso-surface of an (H, W, T) occupancy volume
    (numpy array, or a CUDA tensor that is then not copied to the host) at ``mcubes_thres``, written to ``savename``
    (``.dae`` as in the reference's drivers, ``.obj`` or ``.ply``).  Vertices are in index units, as PyMCubes' are.

    The extraction is ``functional.iso_surface`` on the device -- marching tetrahedra, not PyMCubes' marching cubes: the
    same level set, other triangles.  With ``smoothen`` the volume is binarised at the threshold, shifted by -0.5,
    blurred by a separable Gaussian (sigma = 1, truncated at 4 sigma, edge values replicated; wire_gauss3_blur) and
    cut at 0.  That is NOT PyMCubes' ``smooth`` (the reference's line 431), which blurs a signed distance transform of
    the binary volume: its output cannot be reproduced or compared here.  Returns None, as the reference does."""
    v, f = march(occupancy, mcubes_thres, smoothen)
    save_mesh(v, f, savename)


def export_mesh(coords, cube_res, model, batchsize, savename, occupancy=None, thres=0.005):
    """modules/volutils.py:94-142: ``query_occupancy``, then the iso-surface of the cube at ``thres`` written to
    ``savename`` (see ``march_and_save`` for the formats and for how the mesh differs from PyMCubes').  Returns the
    occupancy cube, as the reference does."""
    occupancy = query_occupancy(coords, cube_res, model, batchsize, occupancy)
    march_and_save(occupancy, thres, savename)
    return occupancy
