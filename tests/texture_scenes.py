"""The host harness of the texture tests (a helper module, not a test file): a ctypes wrapper of
tests/host_harness/mesh_texture_harness.cpp built together with mesh_harness.cpp, the sanitizer program, and the closed-form
scenes tests/test_mesh_texture_host.py and tests/test_gpu_mesh_texture.py share."""
import ctypes
import os
import subprocess

import numpy as np

import mesh_ref as MR
import mesh_scenes as MS
import texture_ref as TR

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = [os.path.join(HERE, "host_harness", n) for n in ("mesh_harness.cpp", "mesh_texture_harness.cpp")]
WRAP = {TR.REPEAT: 0, TR.CLAMP: 1, TR.MIRROR: 2}
FILTER = {"bilinear": 0, "trilinear": 1}
MIP_SIZES = ((1, 1), (2, 2), (5, 3), (7, 1), (17, 17), (64, 32))                   # (w, h)


def build_harness(out_dir, flags=("-O2", "-ffp-contract=off")):
    """The two harness files in one library: mesh_scenes' wrapper of the untextured walk, plus mth_*."""
    so = os.path.join(str(out_dir), "libmesh_texture_harness.so")
    subprocess.run(["g++", *flags, "-std=c++17", "-shared", "-fPIC", *HARNESS, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.mh_rasterize.argtypes = [i, i, p, p, i, p, p, p, p, p, i, p, p, p, i, i, f, f, i, i, f, p, p, p, p, p, p]
    lib.mh_rasterize.restype = i
    lib.mth_layout.argtypes, lib.mth_layout.restype = [i, p, p, p], ctypes.c_uint64
    lib.mth_build_mips.argtypes, lib.mth_build_mips.restype = [i, p, p], None
    lib.mth_resolve.argtypes = [i, i, p, i, p, p, p, p, i, i, i, f, p, p, p, p, i, p, p, ctypes.c_uint64, i, p, p, p, p]
    lib.mth_resolve.restype = i
    return lib


def build_sanitized_program(out_dir):
    """The stand-alone program with its own main under -fsanitize=address,undefined: its path."""
    exe = os.path.join(str(out_dir), "mesh_texture_sanitize")
    main = os.path.join(HERE, "host_harness", "mesh_texture_harness_main.cpp")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-std=c++17", *HARNESS, main, "-o", exe], check=True)
    return exe


_ptr = MS._ptr


def harness_texture_set(lib, textures):
    """(descriptors int32 [T,20], texels uint32 [count]) of a list of (image, wrap_s, wrap_t), mips built by the harness."""
    T = len(textures)
    images = [TR.rgba(t[0]) for t in textures]
    sizes = np.array([[im.shape[1], im.shape[0]] for im in images], np.int32)
    wraps = np.array([[WRAP[t[1]], WRAP[t[2]]] for t in textures], np.int32)
    desc = np.zeros((T, 20), np.int32)
    count = lib.mth_layout(T, _ptr(sizes), _ptr(wraps), _ptr(desc))
    assert count > 0
    texels = np.zeros(count, np.uint32)
    for k, im in enumerate(images):
        at = int(desc[k, 4])
        texels[at:at + im.shape[0] * im.shape[1]] = TR.pack_words(im).reshape(-1)
    lib.mth_build_mips(T, _ptr(desc), _ptr(texels))
    return desc, texels


def harness_render_textured(lib, verts, faces, K, width, height, face_uvs, face_textures, textures, texture_filter, *, near=0.01,
                            far=1e10, vertex_colors=None, face_colors=None, headlight=False, ambient=0.3):
    """One camera-space scene through mh_rasterize and mth_resolve: (plain, textured) dicts of rgb, depth, face_ids, normals
    [H,W,..] -- plain is the untextured walk's output."""
    plain = MS.harness_render(lib, verts, faces, MS.IDENTITY_VIEW, np.asarray(K, np.float32)[None], width, height, near=near, far=far,
                              vertex_colors=vertex_colors, face_colors=face_colors, headlight=headlight, ambient=ambient)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    desc, texels = harness_texture_set(lib, textures)
    faces = np.ascontiguousarray(faces, np.int32)
    uv, ft = f32(face_uvs), np.ascontiguousarray(face_textures, np.int32)
    vcol, fcol, Kc = f32(vertex_colors), f32(face_colors), f32(K).reshape(1, 3, 3)
    out = dict(rgb=np.empty((1, height, width, 3), np.float32), depth=np.empty((1, height, width), np.float32),
               face_ids=np.empty((1, height, width), np.int32), normals=np.empty((1, height, width, 3), np.float32))
    rc = lib.mth_resolve(1, len(verts), _ptr(plain["verts_cam"]), len(faces), _ptr(faces), _ptr(vcol), _ptr(fcol), _ptr(Kc), width,
                         height, int(headlight), float(ambient), _ptr(plain["face_ids"]), _ptr(plain["depth"]), _ptr(uv), _ptr(ft),
                         len(textures), _ptr(desc), _ptr(texels), len(texels), FILTER[texture_filter], _ptr(out["rgb"]),
                         _ptr(out["depth"]), _ptr(out["face_ids"]), _ptr(out["normals"]))
    assert rc == 0
    return {k: v[0] for k, v in plain.items() if k in out}, {k: v[0] for k, v in out.items()}


# ---- closed forms (none of them comes from texture_ref's sampling code) -------------------------------------------------------
def texel_centre_case(minify=1):
    """A fronto-parallel quad over a 16 x 12 image with a (16 minify) x (12 minify) texture, uv 0 .. 1 across: every pixel
    centre lands on a texel centre of level log2(minify).  dict(scene.., W, H, textures, expect float64 [H,W,3])."""
    W, H = 16, 12
    K = MR.pinhole(W, H)
    image = TR.noise_checker(W * minify, H * minify, 77)
    q = TR.quad(K, W, H, z=3.0)
    level = image
    for _ in range(int(np.log2(minify))):                                           # the box filter, as a direct loop
        h, w = level.shape[:2]
        nxt = np.zeros((max(1, h // 2), max(1, w // 2), 4), np.uint8)
        for y in range(nxt.shape[0]):
            for x in range(nxt.shape[1]):
                for ch in range(4):
                    s = sum(int(level[min(2 * y + dy, h - 1), min(2 * x + dx, w - 1), ch]) for dy in (0, 1) for dx in (0, 1))
                    nxt[y, x, ch] = (s + 2) >> 2
        level = nxt
    assert level.shape[:2] == (H, W)
    return dict(q, K=K, W=W, H=H, face_textures=np.zeros(2, np.int32), textures=[(image, TR.CLAMP, TR.CLAMP)],
                expect=level[..., :3].astype(np.float64) / 255.0)


def ramp_case():
    """A quad tilted in depth (z 2 on the left, 5 on the right) over a 32 x 8 image with a 256 x 2 ramp, byte = column:
    bilinear gives rgb = (256 u - 0.5) / 255 in the interior, u the perspective-correct coordinate, here from the ray-plane
    intersection.  dict(.., expect [H,W] float64, interior bool [H,W])."""
    W, H = 32, 8
    K = MR.pinhole(W, H)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 2, 0).repeat(4, 2)
    q = TR.quad(K, W, H, z=2.0, z_right=5.0)
    v = q["verts"].astype(np.float64)
    a, ex, ey = v[0], v[1] - v[0], v[3] - v[0]
    nrm = np.cross(ex, ey)
    y, x = np.mgrid[0:H, 0:W]
    ray = np.stack([((x + 0.5) - K[0, 2]) / K[0, 0], ((y + 0.5) - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    P = ray * ((nrm @ a) / (ray @ nrm))[..., None]
    # the left and the right edge are both parallel to Y (a trapezoid in one plane), u is 0 on the one and 1 on the other: it
    # is the position along ex in the XZ projection, where the plane is a line
    u = ((P[..., 0] - a[0]) * ex[0] + (P[..., 2] - a[2]) * ex[2]) / (ex[0] ** 2 + ex[2] ** 2)
    expect = (256.0 * u - 0.5) / 255.0
    return dict(q, K=K, W=W, H=H, face_textures=np.zeros(2, np.int32), textures=[(ramp, TR.CLAMP, TR.CLAMP)], expect=expect,
                interior=(u > 1.0 / 256) & (u < 1 - 1.0 / 256), u=u)
