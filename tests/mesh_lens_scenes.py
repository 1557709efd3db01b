"""The host harness and the scenes of the lens mesh rasteriser's tests (a helper module, not a test file): a ctypes wrapper of
tests/host_harness/mesh_lens_harness.cpp and the cases tests/test_mesh_lens_host.py and tests/test_gpu_mesh_lens.py share."""
import ctypes
import os
import subprocess

import numpy as np

import mesh_lens_ref as ML
import mesh_ref as MR

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "host_harness", "mesh_lens_harness.cpp")
SIZES = [(37, 29), (112, 80)]


def build_harness(out_dir, flags=("-O2", "-ffp-contract=off")):
    so = os.path.join(str(out_dir), "libmesh_lens_harness.so")
    subprocess.run(["g++", *flags, "-std=c++17", "-shared", "-fPIC", HARNESS, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.mlh_rays.argtypes = [i, i, p, i, i, p, p, p]
    lib.mlh_rays.restype = None
    lib.mlh_rasterize.argtypes = [i, i, p, p, i, p, p, p, p, i, p, i, p, p, p, i, i, f, f, i, i, f, p, i, p, p, p, p, p, p, p, p]
    lib.mlh_rasterize.restype = i
    lib.mlh_workspace_layout.argtypes = [i, i, i, p]
    lib.mlh_workspace_layout.restype = None
    lib.mlh_distort.argtypes = [i, p, f, f, p]
    lib.mlh_distort.restype = None
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def table_shapes(width, height):
    """((BY, BX), (SY, SX)) of include/mgs_mesh_lens.h."""
    bx, by = (width + 7) // 8, (height + 7) // 8
    return (by, bx), ((by + 7) // 8, (bx + 7) // 8)


def harness_rays(lib, model, rows, width, height):
    """mlh_rays: (rays [C,H,W,2], blocks [C,BY,BX,4], supers [C,SY,SX,4]) float32."""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 16)
    C = len(rows)
    bs, ss = table_shapes(width, height)
    rays = np.empty((C, height, width, 2), np.float32)
    blocks, supers = np.empty((C,) + bs + (4,), np.float32), np.empty((C,) + ss + (4,), np.float32)
    lib.mlh_rays(C, int(model), _ptr(rows), width, height, _ptr(rays), _ptr(blocks), _ptr(supers))
    return rays, blocks, supers


def harness_render(lib, verts, faces, viewmats, model, rows, width, height, *, vertex_colors=None, face_colors=None, near=0.01,
                   far=1e10, cull=False, headlight=False, ambient=0.3, rays=None, every_block=False):
    """mlh_rasterize: dict(verts_cam [C,V,3], rgb [C,H,W,3], depth, face_ids [C,H,W], normals [C,H,W,3], rays [C,H,W,2] (the
    map used: `rays` where given), listed [C], keys [C], face_blocks [C,F])."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    verts, viewmats, rows = f32(verts), f32(viewmats).reshape(-1, 4, 4), f32(rows).reshape(-1, 16)
    faces = np.ascontiguousarray(faces, np.int32)
    vertex_colors, face_colors, rays = f32(vertex_colors), f32(face_colors), f32(rays)
    C, V, F = len(viewmats), len(verts), len(faces)
    assert len(rows) == C and (rays is None or rays.shape == (C, height, width, 2))
    out = dict(verts_cam=np.empty((C, V, 3), np.float32), rgb=np.empty((C, height, width, 3), np.float32),
               depth=np.empty((C, height, width), np.float32), face_ids=np.empty((C, height, width), np.int32),
               normals=np.empty((C, height, width, 3), np.float32), rays=np.empty((C, height, width, 2), np.float32),
               face_blocks=np.zeros((C, F), np.int32))
    stats = np.zeros((C, 2), np.int64)
    rc = lib.mlh_rasterize(C, V, _ptr(verts), None, 0, None, None, None, _ptr(viewmats), int(model), _ptr(rows), F, _ptr(faces),
                           _ptr(vertex_colors), _ptr(face_colors), width, height, float(near), float(far), int(cull),
                           int(headlight), float(ambient), _ptr(rays), int(every_block), _ptr(out["verts_cam"]), _ptr(out["rgb"]),
                           _ptr(out["depth"]), _ptr(out["face_ids"]), _ptr(out["normals"]), _ptr(out["rays"]), _ptr(stats),
                           _ptr(out["face_blocks"]))
    assert rc == 0
    out["listed"], out["keys"] = stats[:, 0].copy(), stats[:, 1].copy()
    return out


def camera(lens, width, height):
    """(model, coefficients, K float32 [3,3], row float32 [16]) of a test lens at width x height."""
    model, k, _ = ML.LENSES[lens]
    K = ML.intrinsics(lens, width, height)
    return model, k, K, ML.lens_row(lens, K)[1]


def spanning_cases(lens, width, height):
    """name -> dict(verts, faces[, near]): the faces the box's conservativeness is held on besides mesh_ref.raster_cases -- a
    triangle crossing the near plane that spans the frame, faces straddling the frame's edge, and faces straddling the fold
    (the border of the rays the lens has; under a lens without a fold in the frame they straddle the frame's corner rays)."""
    model, k, K, _ = camera(lens, width, height)
    ref = ML.RayRef(model, K, k, width, height)
    q = ref.q.reshape(-1, 2)[ref.valid.reshape(-1)]
    lo, hi = q.min(0), q.max(0)
    span = hi - lo
    cases = {}
    # two vertices at z = 3, one behind the camera: clipped at near = 0.5 its rays reach from -L/3 to L/2 in y and past
    # +-L/3 in x, L ten times the largest ray coordinate of the frame
    L = 10.0 * float(np.abs(q).max())
    cases["near_crossing_spans_frame"] = dict(verts=np.array([[-L, -L, 3.0], [L, -L, 3.0], [0.0, L, -1.0]], np.float32),
                                              faces=np.array([[0, 1, 2]], np.int32), near=0.5)
    rng = np.random.default_rng(5)
    edge = []
    for i in range(24):                                   # centres on the border of the rays' box: half in, half out
        t = rng.uniform(0, 1)
        c = [(lo[0] + t * span[0], lo[1]), (lo[0] + t * span[0], hi[1]), (lo[0], lo[1] + t * span[1]), (hi[0], lo[1] + t * span[1])][i % 4]
        edge.append(np.array(c)[None] + rng.normal(scale=0.08 * span.max(), size=(3, 2)))
    xy = np.concatenate(edge)
    zz = np.repeat(rng.uniform(2.0, 5.0, 24), 3)
    cases["straddle_frame_edge"] = dict(verts=np.concatenate([xy * zz[:, None], zz[:, None]], 1).astype(np.float32),
                                        faces=np.arange(72, dtype=np.int32).reshape(-1, 3))
    # the fold: the valid rays furthest from the axis, faces centred on them and reaching past them
    r = np.hypot(q[:, 0], q[:, 1])
    far_rays = q[np.argsort(r)[-24:]]
    fold = [c[None] * rng.uniform(0.97, 1.08) + rng.normal(scale=0.06 * span.max(), size=(3, 2)) for c in far_rays]
    xy = np.concatenate(fold)
    cases["straddle_fold"] = dict(verts=np.concatenate([xy * zz[:, None], zz[:, None]], 1).astype(np.float32),
                                  faces=np.arange(72, dtype=np.int32).reshape(-1, 3))
    for c in cases.values():
        c.setdefault("near", 0.01), c.setdefault("far", 1e10), c.setdefault("cull", False)
    return cases


def threshold_candidates(lens, width, height, n=160, seed=9):
    """n right triangles of growing size around the frame's centre rays, one depth each: among them the harness finds boxes of
    14, 15 and 16 blocks."""
    model, k, K, _ = camera(lens, width, height)
    rng = np.random.default_rng(seed)
    f = float(K[0, 0])
    verts = []
    for i in range(n):
        # (every third one thin and tall: 14 blocks is 2 x 7)
        w, h = (rng.uniform(8, 15) / f, rng.uniform(47, 56) / f) if i % 3 == 0 else (rng.uniform(10, 40) / f, rng.uniform(10, 52) / f)
        c = rng.uniform(-6, 6, 2) / f
        z = 3.0 + 0.01 * i
        uv = np.array([[c[0] - w / 2, c[1] - h / 2], [c[0] + w / 2, c[1] - h / 2], [c[0] - w / 2, c[1] + h / 2]])
        verts.append(np.concatenate([uv * z, np.full((3, 1), z)], 1))
    return np.concatenate(verts).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
