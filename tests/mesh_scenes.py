"""Scenes and the host harness of the mesh rasteriser's tests (a helper module, not a test file): the open box of the pin
with its six cameras, the posed box, the wide image, the 1920 x 1080 versions and the close-up with more than a thousand
faces on the large-face path, the scene-file writer of scripts/mesh_host_sanitize.py and a ctypes wrapper of
tests/host_harness/mesh_harness.cpp.  tests/test_mesh_raster_host.py, tests/test_gpu_mesh.py and the scripts share them."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import mesh_ref as MR

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = {"top": 5, "bottom": 0, "front": 3, "back": 1, "left": 4, "right": 2}      # tests/test_mesh_host.py: xor pixels against the reference
MAGIC = 0x4853454D
LARGE_BLOCKS = 15                                                                 # MGS_MESH_LARGE_BLOCKS


def openbox():
    """dict(verts float32 [V,3] (lid first), faces int32 [F,3], n_lid, views name -> dict(viewmat [4,4], K [3,3], silhouette
    bool [800,800]), hinge_point, hinge_axis): tests/golden/mesh_openbox.npz under the pin's camera convention."""
    g = np.load(os.path.join(HERE, "golden", "mesh_openbox.npz"))
    cam = np.load(os.path.join(HERE, "golden", "camera_reference.npz"))
    verts = np.concatenate([g["lid_vertices"], g["body_vertices"]]).astype(np.float32)
    faces = np.concatenate([g["lid_faces"].astype(np.int32), g["body_faces"].astype(np.int32) + len(g["lid_vertices"])])
    names = [str(n) for n in cam["cam_names"]]
    views = {}
    for k, name in enumerate(str(n) for n in g["sil_names"]):
        i = names.index(name)
        viewmat = (np.diag([1.0, -1.0, -1.0, 1.0]) @ np.linalg.inv(cam["cam_c2w"][i])).astype(np.float32)
        h, w = (int(v) for v in g["sil_shape"])
        sil = np.unpackbits(g["sil_bits"][k])[:h * w].reshape(h, w).astype(bool)
        views[name] = dict(viewmat=viewmat, K=cam["cam_K"][i].astype(np.float32), silhouette=sil)
    link = np.full(len(verts), -1, np.int32)
    link[:len(g["lid_vertices"])] = 0
    return dict(verts=verts, faces=faces, n_lid=len(g["lid_vertices"]), views=views, link_ids=link)


def hinge_of_openbox():
    """(point, unit axis) float64 of the hinge recorded in tests/golden/hinge_openbox.npz."""
    h = np.load(os.path.join(HERE, "golden", "hinge_openbox.npz"))
    point, axis = np.asarray(h["position"], np.float64), np.asarray(h["axis"], np.float64)
    return point, axis / np.linalg.norm(axis)


def rotation_about(axis, angle):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(angle) * np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * np.outer(k, k)


def lid_pose(angle=0.6):
    """(R [1,3,3], t [1,3]) float32: the lid turned by `angle` about the recorded hinge, t = p - R p."""
    p, axis = hinge_of_openbox()
    R = rotation_about(axis, angle)
    return R[None].astype(np.float32), (p - R @ p)[None].astype(np.float32)


def scaled_K(K, sx, sy=None):
    """K with its first two rows scaled: the same view at sx x sy times the resolution."""
    K = np.array(K, np.float32)
    K[0] *= np.float32(sx)
    K[1] *= np.float32(sx if sy is None else sy)
    return K


def top_1080p(box):
    """(viewmat, K) of the pin's `top` camera rescaled to 1920 x 1080: the 800 x 800 view scaled by 1.35 (the height) and
    centred."""
    v = box["views"]["top"]
    K = scaled_K(v["K"], 1.35)
    K[0, 2] += np.float32((1920 - 1080) / 2)
    return v["viewmat"], K


def closeup_1080p(box, zoom=16.0):
    """(viewmat, K) at 1920 x 1080: the `top` camera zoomed `zoom` times onto the middle of the lid, so that the 2-pixel
    faces of the 800 x 800 view become boxes of about five blocks a side: more than a thousand of them are in view and
    every one is past the large-face threshold."""
    v = box["views"]["top"]
    cam, _ = MR.vertex_ref(box["verts"][:box["n_lid"]], None, None, None, None, v["viewmat"][None])
    c = np.median(cam[0], axis=0)
    K = np.array(v["K"], np.float64)
    u0, v0 = K[0, 0] * c[0] / c[2] + K[0, 2], K[1, 1] * c[1] / c[2] + K[1, 2]
    Kz = K.copy()
    Kz[0, 0], Kz[1, 1] = K[0, 0] * zoom, K[1, 1] * zoom
    Kz[0, 2], Kz[1, 2] = 960.0 - zoom * (u0 - K[0, 2]), 540.0 - zoom * (v0 - K[1, 2])
    return v["viewmat"], Kz.astype(np.float32)


def wide_case():
    """The 2064 x 16 image (258 blocks across): one triangle over the whole image plus 64 random faces, camera space."""
    W, H = 2064, 16
    K = MR.pinhole(W, H)
    v, f = MR.random_faces(64, W, H, seed=21, K=K)
    big = np.array([[-40, -30, 4.0], [40, -30, 4.0], [0, 50, 4.0]], np.float32)
    return dict(verts=np.concatenate([big, v]), faces=np.concatenate([[[0, 1, 2]], f + 3]).astype(np.int32), K=K, width=W,
                height=H, near=0.01, far=1e10, cull=False)


def own_threshold_case(width=64, height=64):
    """Boxes of LARGE_BLOCKS - 1, LARGE_BLOCKS and LARGE_BLOCKS + 1 blocks (2 x 7, 3 x 5, 4 x 4), overlapping, at three depths:
    raster_cases' threshold_blocks, kept beside it so that a change of the threshold has to change this line."""
    K = MR.pinhole(width, height)
    shapes = {14: (2, 7), 15: (3, 5), 16: (4, 4)}
    v = np.concatenate([MR.box_in_blocks(1 + i, 0, *shapes[n], K, z=3.0 + i)
                        for i, n in enumerate((LARGE_BLOCKS - 1, LARGE_BLOCKS, LARGE_BLOCKS + 1))])
    return dict(verts=v, faces=np.arange(9, dtype=np.int32).reshape(3, 3), K=K, near=0.01, far=1e10, cull=False)


# ---- the host harness ---------------------------------------------------------------------------------------------------
def build_harness(out_dir, flags=("-O2", "-ffp-contract=off")):
    so = os.path.join(str(out_dir), "libmesh_harness.so")
    subprocess.run(["g++", *flags, "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "host_harness", "mesh_harness.cpp"),
                    "-o", so], check=True)
    lib = ctypes.CDLL(so)
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.mh_rasterize.argtypes = [i, i, p, p, i, p, p, p, p, p, i, p, p, p, i, i, f, f, i, i, f, p, p, p, p, p, p]
    lib.mh_rasterize.restype = i
    lib.mh_workspace_layout.argtypes = [i, i, i, i, p]
    lib.mh_workspace_layout.restype = None
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def harness_render(lib, verts, faces, viewmats, Ks, width, height, *, link_ids=None, rotations=None, translations=None,
                   scales=None, vertex_colors=None, face_colors=None, near=0.01, far=1e10, cull=False, headlight=False,
                   ambient=0.3):
    """mh_rasterize: dict(verts_cam [C,V,3], rgb [C,H,W,3], depth, face_ids [C,H,W], normals [C,H,W,3], listed [C]: the faces
    on the camera's large-face list, keys [C]: the (pixel, face) pairs that reached the visibility update)."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    verts, viewmats, Ks = f32(verts), f32(viewmats).reshape(-1, 4, 4), f32(Ks).reshape(-1, 3, 3)
    faces = np.ascontiguousarray(faces, np.int32)
    link_ids = None if link_ids is None else np.ascontiguousarray(link_ids, np.int32)
    rotations, translations, scales = f32(rotations), f32(translations), f32(scales)
    vertex_colors, face_colors = f32(vertex_colors), f32(face_colors)
    C, V, F, L = len(viewmats), len(verts), len(faces), 0 if rotations is None else len(rotations)
    out = dict(verts_cam=np.empty((C, V, 3), np.float32), rgb=np.empty((C, height, width, 3), np.float32),
               depth=np.empty((C, height, width), np.float32), face_ids=np.empty((C, height, width), np.int32),
               normals=np.empty((C, height, width, 3), np.float32))
    stats = np.zeros((C, 2), np.int64)
    rc = lib.mh_rasterize(C, V, _ptr(verts), _ptr(link_ids), L, _ptr(rotations), _ptr(translations), _ptr(scales),
                          _ptr(viewmats), _ptr(Ks), F, _ptr(faces), _ptr(vertex_colors), _ptr(face_colors), width, height,
                          float(near), float(far), int(cull), int(headlight), float(ambient), _ptr(out["verts_cam"]),
                          _ptr(out["rgb"]), _ptr(out["depth"]), _ptr(out["face_ids"]), _ptr(out["normals"]), _ptr(stats))
    assert rc == 0
    out["listed"], out["keys"] = stats[:, 0].copy(), stats[:, 1].copy()
    return out


def write_scene(fh, verts, faces, viewmats, Ks, width, height, *, link_ids=None, rotations=None, translations=None,
                scales=None, vertex_colors=None, face_colors=None, near=0.01, far=1e10, cull=False, headlight=False,
                ambient=0.3):
    """One scene in the format tests/host_harness/mesh_harness_main.cpp reads."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    viewmats, Ks = f32(viewmats).reshape(-1, 4, 4), f32(Ks).reshape(-1, 3, 3)
    L = 0 if rotations is None else len(rotations)
    fh.write(struct.pack("<12i", MAGIC, len(viewmats), len(verts), len(faces), L, width, height, int(cull), int(headlight),
                         int(vertex_colors is not None), int(face_colors is not None), int(link_ids is not None)))
    fh.write(struct.pack("<3f", near, far, ambient))
    fh.write(f32(verts).tobytes())
    fh.write(np.ascontiguousarray(faces, np.int32).tobytes())
    if link_ids is not None:
        fh.write(np.ascontiguousarray(link_ids, np.int32).tobytes())
    if L:
        fh.write(f32(rotations).tobytes())
        fh.write(f32(translations).tobytes())
        fh.write(f32(np.ones(L) if scales is None else scales).tobytes())
    fh.write(viewmats.tobytes())
    fh.write(Ks.tobytes())
    if vertex_colors is not None:
        fh.write(f32(vertex_colors).tobytes())
    if face_colors is not None:
        fh.write(f32(face_colors).tobytes())


IDENTITY_VIEW = np.eye(4, dtype=np.float32)[None]


# ---- checks shared by the host and the GPU tests ----------------------------------------------------------------------------
def check_shading(R, r, faces, rgb, normals=None, vertex_colors=None, face_colors=None, headlight=False, ambient=0.3):
    """Hold rgb [H,W,3] (and normals) of one camera to RasterRef.shade_ref at the winners check_raster returned: error over
    bound <= 1 at every covered pixel (the normal's sign is free where flip_open), exact zeros at every other pixel.
    Returns the worst ratios."""
    ref = R.shade_ref(r["pairs"], r["pixels"], faces, vertex_colors=vertex_colors, face_colors=face_colors,
                      headlight=headlight, ambient=ambient)
    n_px = R.width * R.height
    rgb = np.asarray(rgb, np.float64).reshape(n_px, 3)
    un = np.ones(n_px, bool)
    un[r["pixels"]] = False
    assert (rgb[un] == 0).all(), "rgb is not exactly 0 where uncovered"
    worst = {"rgb": 0.0, "normal": 0.0}
    if len(r["pixels"]):
        ratio = np.abs(rgb[r["pixels"]] - ref["rgb"]) / ref["tol_rgb"]
        worst["rgb"] = float(ratio.max())
        assert worst["rgb"] <= 1, f"rgb off its bound: worst ratio {worst['rgb']:.3g}"
    if normals is not None:
        n = np.asarray(normals, np.float64).reshape(n_px, 3)
        assert (n[un] == 0).all(), "normals are not exactly 0 where uncovered"
        if len(r["pixels"]):
            got, tn = n[r["pixels"]], ref["tol_normal"][:, None]
            same = np.abs(got - ref["normal"]) / tn
            flipped = np.abs(got + ref["normal"]) / tn
            ratio = np.where(ref["flip_open"][:, None], np.minimum(same, flipped), same)
            worst["normal"] = float(ratio.max())
            assert worst["normal"] <= 1, f"normal off its bound: worst ratio {worst['normal']:.3g}"
    return worst


def check_pin(R, face_ids, silhouette, name):
    """(xor, d): the coverage's xor against the reference's silhouette and the pixels d whose coverage differs from the
    fp64 statement's; asserts xor <= PIN[name] + d."""
    cov = np.asarray(face_ids).reshape(R.height, R.width) >= 0
    d = int((cov != R.mask()).sum())
    xor = int((cov ^ silhouette).sum())
    assert xor <= PIN[name] + d, (name, xor, d)
    return xor, d
