"""Textured meshes without a GPU: the fp64 statement (tests/texture_ref.py) against closed forms that do not come from it,
its mip chain against a direct loop, the 5 % cap on every scene the GPU tests use, the host build of
robosimgs_amd/csrc/mesh_texture.h (tests/host_harness/mesh_texture_harness.cpp) against the statement, a stand-alone
program of the same code under -fsanitize=address,undefined on the hostile inputs, the C ABI's refusals, and the loaders."""
import ctypes
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mesh_ref as MR
import mesh_scenes as MS
import texture_ref as TR
import texture_scenes as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(37, 29), (64, 64)]
FILTERS = ["bilinear", "trilinear"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return TS.build_harness(tmp_path_factory.mktemp("mesh_texture_harness"))


def _ref_render(c, W, H):
    """(RasterRef, r) with the reference's own winners as the "kernel output"."""
    R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H)
    return R, R.check_raster(R.winner.reshape(H, W), R.zwin.reshape(H, W))


# ---- the statement against closed forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("texture_filter", FILTERS)
@pytest.mark.parametrize("minify", [1, 2])
def test_statement_returns_the_texel_where_pixel_centres_land_on_texel_centres(texture_filter, minify):
    """minify 1: the texture's bytes / 255 under both filters.  minify 2: trilinear returns level 1 (lod = 1); bilinear reads
    level 0 between four texels, whose mean is level 1 up to the box filter's integer rounding, half a byte."""
    c = TS.texel_centre_case(minify)
    R, r = _ref_render(c, c["W"], c["H"])
    assert r["covered"] == c["W"] * c["H"]
    ref = TR.shade_textured_ref(R, r["pairs"], r["pixels"], c["faces"], c["face_uvs"], c["face_textures"], c["textures"], texture_filter)
    assert ref["textured"].all()
    slack = 1e-5 if (minify == 1 or texture_filter == "trilinear") else 0.5 / 255 + 1e-5
    got = np.zeros((c["H"] * c["W"], 3))
    got[r["pixels"]] = ref["rgb"]
    assert np.abs(got.reshape(c["H"], c["W"], 3) - c["expect"]).max() <= slack
    if texture_filter == "trilinear":
        assert np.abs(ref["lod"] - np.log2(minify)).max() <= 1e-5
    assert ref["tol_rgb"].max() <= TR.CAP_TOL


def test_statement_interpolates_perspective_correctly_on_a_tilted_ramp():
    c = TS.ramp_case()
    R, r = _ref_render(c, c["W"], c["H"])
    ref = TR.shade_textured_ref(R, r["pairs"], r["pixels"], c["faces"], c["face_uvs"], c["face_textures"], c["textures"], "bilinear")
    got = np.full((c["H"] * c["W"], 3), np.nan)
    got[r["pixels"]] = ref["rgb"]
    got = got.reshape(c["H"], c["W"], 3)
    inside = c["interior"]
    assert inside.sum() > 0.9 * inside.size
    assert np.abs(got[inside] - c["expect"][inside][:, None]).max() <= 1e-5
    # an affine (screen-space) interpolation would be off by far more than that in the middle of the quad
    assert np.abs((np.arange(c["W"]) + 0.5) / c["W"] - c["u"][0]).max() > 0.1


@pytest.mark.parametrize("size", TS.MIP_SIZES)
def test_mip_chain_matches_a_direct_loop(size, harness):
    w, h = size
    img = np.random.default_rng(w * 100 + h).integers(0, 256, (h, w, 4)).astype(np.uint8)
    chain = TR.mip_chain(img)
    assert len(chain) == 1 + int(np.floor(np.log2(max(w, h)))) and chain[-1].shape[:2] == (1, 1)
    for l in range(1, len(chain)):
        src = chain[l - 1].astype(int)
        sh, sw = src.shape[:2]
        assert chain[l].shape == (max(1, h >> l), max(1, w >> l), 4)
        for y in range(chain[l].shape[0]):
            for x in range(chain[l].shape[1]):
                ys, xs = (min(2 * y, sh - 1), min(2 * y + 1, sh - 1)), (min(2 * x, sw - 1), min(2 * x + 1, sw - 1))
                want = (sum(src[yy, xx] for yy in ys for xx in xs) + 2) >> 2
                assert (chain[l][y, x] == want).all(), (l, x, y)
    # the host build of the kernel's code gives the same bytes, level by level
    desc, texels = TS.harness_texture_set(harness, [(img, TR.REPEAT, TR.REPEAT)])
    assert desc[0, 2] == len(chain) and len(texels) == sum(c.shape[0] * c.shape[1] for c in chain)
    for l, level in enumerate(chain):
        at = int(desc[0, 4 + l])
        assert np.array_equal(texels[at:at + level.shape[0] * level.shape[1]], TR.pack_words(level).reshape(-1)), l


# ---- the cap, on every scene the GPU tests use --------------------------------------------------------------------------------
def _scenes(W, H):
    yield "random", TR.random_textured_scene(W, H), {}
    yield "mixed", TR.random_textured_scene(W, H, untextured_every=2), dict(vertex_colors=np.random.default_rng(5).uniform(0, 1, (387, 3)).astype(np.float32))


@pytest.mark.parametrize("size", SIZES)
def test_at_most_five_percent_of_textured_pixels_have_a_bound_above_4_255(size):
    W, H = size
    for name, c, shade in _scenes(W, H):
        R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H)
        assert R.tolerance_share() <= 0.02
        r = R.check_raster(R.winner.reshape(H, W), R.zwin.reshape(H, W))
        for wraps in ((TR.REPEAT, TR.CLAMP, TR.MIRROR), (TR.CLAMP, TR.MIRROR, TR.REPEAT), (TR.MIRROR, TR.REPEAT, TR.CLAMP)):
            for texture_filter in FILTERS:
                for light in (dict(), dict(headlight=True, ambient=0.25)):
                    ref = TR.shade_textured_ref(R, r["pairs"], r["pixels"], c["faces"], c["face_uvs"], c["face_textures"],
                                                TR.scene_textures(wraps), texture_filter, **shade, **light)
                    strict = ~R.by_tolerance[r["pixels"]]
                    share = TR.cap_share(ref, strict)
                    assert (ref["textured"] & strict).sum() >= 20
                    assert share <= TR.CAP_SHARE, (name, size, wraps, texture_filter, share)
    for c in (TS.texel_centre_case(1), TS.texel_centre_case(2), TS.ramp_case()):
        R, r = _ref_render(c, c["W"], c["H"])
        for texture_filter in FILTERS:
            ref = TR.shade_textured_ref(R, r["pairs"], r["pixels"], c["faces"], c["face_uvs"], c["face_textures"], c["textures"],
                                        texture_filter)
            assert TR.cap_share(ref) <= TR.CAP_SHARE


# ---- the host build of the shared header against the statement -----------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_harness_stays_inside_the_counted_bound_and_leaves_the_raster_outputs_alone(harness, size):
    W, H = size
    for name, c, shade in _scenes(W, H):
        R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H)
        for k, wraps in enumerate(((TR.REPEAT, TR.CLAMP, TR.MIRROR), (TR.CLAMP, TR.MIRROR, TR.REPEAT), (TR.MIRROR, TR.REPEAT, TR.CLAMP))):
            tex = TR.scene_textures(wraps)
            for texture_filter in FILTERS:
                light = dict(headlight=True, ambient=0.25) if k == 1 else {}
                plain, out = TS.harness_render_textured(harness, c["verts"], c["faces"], c["K"], W, H, c["face_uvs"], c["face_textures"],
                                                        tex, texture_filter, **shade, **light)
                for key in ("depth", "face_ids", "normals"):
                    assert np.array_equal(out[key].view(np.int32), plain[key].view(np.int32)), key
                r = R.check_raster(out["face_ids"], out["depth"])
                res = TR.check_textured_shading(R, r, c["faces"], out["rgb"], c["face_uvs"], c["face_textures"], tex, texture_filter,
                                                **shade, **light)
                assert res["textured"] >= 20
                # pixels of untextured faces: the untextured walk's bits
                ids = out["face_ids"]
                un = (ids >= 0) & (np.asarray(c["face_textures"])[np.maximum(ids, 0)] < 0)
                assert np.array_equal(out["rgb"][un].view(np.int32), plain["rgb"][un].view(np.int32))
                if name == "mixed":
                    assert un.sum() >= 20
                print(f"\n{name} {W}x{H} {wraps[0]} {texture_filter}: worst rgb ratio {res['worst']:.3f}, textured {res['textured']}")


@pytest.mark.parametrize("texture_filter", FILTERS)
def test_harness_on_the_closed_forms(harness, texture_filter):
    for c in (TS.texel_centre_case(1), TS.texel_centre_case(2)):
        plain, out = TS.harness_render_textured(harness, c["verts"], c["faces"], c["K"], c["W"], c["H"], c["face_uvs"],
                                                c["face_textures"], c["textures"], texture_filter)
        R = MR.RasterRef(c["verts"], c["faces"], c["K"], c["W"], c["H"])
        r = R.check_raster(out["face_ids"], out["depth"])
        TR.check_textured_shading(R, r, c["faces"], out["rgb"], c["face_uvs"], c["face_textures"], c["textures"], texture_filter)
        if texture_filter == "trilinear" or c["textures"][0][0].shape[1] == c["W"]:
            assert np.abs(out["rgb"] - c["expect"]).max() <= 1e-5
    c = TS.ramp_case()
    plain, out = TS.harness_render_textured(harness, c["verts"], c["faces"], c["K"], c["W"], c["H"], c["face_uvs"], c["face_textures"],
                                            c["textures"], "bilinear")
    assert np.abs(out["rgb"][c["interior"]] - c["expect"][c["interior"]][:, None]).max() <= 1e-5


def test_all_untextured_and_hostile_inputs_in_the_harness(harness):
    W, H = 37, 29
    c = TR.random_textured_scene(W, H)
    tex = TR.scene_textures()
    none = np.full(len(c["faces"]), -1, np.int32)
    for ids in (none, np.full(len(c["faces"]), 3, np.int32), np.full(len(c["faces"]), 2 ** 31 - 1, np.int32), none - 6):
        plain, out = TS.harness_render_textured(harness, c["verts"], c["faces"], c["K"], W, H, c["face_uvs"], ids, tex, "trilinear",
                                                headlight=True)
        for key in ("rgb", "depth", "face_ids", "normals"):
            assert np.array_equal(out[key].view(np.int32), plain[key].view(np.int32)), key
    for bad in (np.nan, np.inf, -np.inf):                                           # a non-finite uv: shaded untextured
        uv = c["face_uvs"].copy()
        uv[:, 1, 0] = bad
        plain, out = TS.harness_render_textured(harness, c["verts"], c["faces"], c["K"], W, H, uv, c["face_textures"], tex, "trilinear")
        assert np.array_equal(out["rgb"].view(np.int32), plain["rgb"].view(np.int32))
    for bad in (1e30, -1e30):                                                       # finite: wrapped, and a colour of the texture
        uv = c["face_uvs"].copy()
        uv[:, 2, 1] = bad
        plain, out = TS.harness_render_textured(harness, c["verts"], c["faces"], c["K"], W, H, uv, c["face_textures"], tex, "trilinear")
        R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H)
        r = R.check_raster(out["face_ids"], out["depth"])
        TR.check_textured_shading(R, r, c["faces"], out["rgb"], uv, c["face_textures"], tex, "trilinear")
        assert np.isfinite(out["rgb"]).all() and out["rgb"].min() >= 0 and out["rgb"].max() <= 1


def test_sanitized_program_passes_the_hostile_inputs(tmp_path):
    exe = TS.build_sanitized_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no sanitizer report" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_abi_header_library_and_binding_agree_and_refuse_bad_arguments():
    from robosimgs_amd import _lib
    from robosimgs_amd.csrc import build
    assert "mesh_texture.hip" in build.SOURCES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgs_mesh_texture.h")).read(), flags=re.S)
    decl = {name: len([a for a in args.split(",") if a.strip()])
            for name, args in re.findall(r"\bint\s+(mgs_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}
    assert sorted(decl) == sorted(_lib.MESH_TEXTURE_EXPORTS) and len(decl) == 4
    assert not set(decl) & set(_lib.MESH_EXPORTS) and "MGS_VERSION" not in src
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for L, path in ((_lib.lib(), _lib.LIB_PATH), (_lib.debug_lib(), _lib.DEBUG_LIB_PATH)):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs and name in nm(path), name
    L = _lib.lib()
    msg = lambda: L.mgs_last_error_string()
    n = ctypes.c_size_t(0)
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)
    desc = (ctypes.c_int32 * 60)()
    assert L.mgs_mesh_texture_layout(3, arr(1, 1, 5, 3, 64, 32), arr(0, 1, 2, 0, 1, 2), desc, ctypes.byref(n)) == 0
    d = np.frombuffer(desc, np.int32).reshape(3, 20)
    assert n.value == 1 + (15 + 2 + 1) + (2048 + 512 + 128 + 32 + 8 + 2 + 1)
    assert d[:, :4].tolist() == [[1, 1, 1, 0 | 1 << 8], [5, 3, 3, 2 | 0 << 8], [64, 32, 7, 1 | 2 << 8]]
    assert d[1, 4:8].tolist() == [1, 16, 18, 0] and d[2, 4:12].tolist() == [19, 2067, 2579, 2707, 2739, 2747, 2749, 0]
    assert L.mgs_mesh_texture_layout(1, arr(16385, 1), None, None, ctypes.byref(n)) == -1 and b"16384" in msg()
    assert L.mgs_mesh_texture_layout(1, arr(0, 1), None, None, ctypes.byref(n)) == -1 and b"16384" in msg()
    assert L.mgs_mesh_texture_layout(4097, arr(1, 1), None, None, ctypes.byref(n)) == -1 and b"4096" in msg()
    assert L.mgs_mesh_texture_layout(0, arr(1, 1), None, None, ctypes.byref(n)) == -1 and b"4096" in msg()
    assert L.mgs_mesh_texture_layout(1, arr(4, 4), arr(3, 0), None, ctypes.byref(n)) == -1 and b"wrap" in msg()
    assert L.mgs_mesh_texture_layout(1, None, None, None, ctypes.byref(n)) == -1 and b"null" in msg()
    big = arr(*([16384, 16384] * 7))                                                # (4^15 - 1) / 3 texels each: six are 2^31 - 2
    assert L.mgs_mesh_texture_layout(7, big, None, None, ctypes.byref(n)) == -1 and b"2^31" in msg()
    assert L.mgs_mesh_texture_layout(6, big, None, None, ctypes.byref(n)) == 0 and n.value == 2 ** 31 - 2
    # build_mips: every call below is refused before a launch (the texel pointer is never dereferenced)
    total = 1 + 18 + 2731
    assert L.mgs_mesh_build_mips(3, desc, None, total, None) == -1 and b"null" in msg()
    assert L.mgs_mesh_build_mips(3, desc, 0x1002, total, None) == -1 and b"aligned" in msg()
    assert L.mgs_mesh_build_mips(3, desc, 0x1000, total - 1, None) == -1 and b"texel_count" in msg()
    bad = (ctypes.c_int32 * 60)(*desc)
    bad[20 + 5] = 17
    assert L.mgs_mesh_build_mips(3, bad, 0x1000, total, None) == -1 and b"layout" in msg()
    bad = (ctypes.c_int32 * 60)(*desc)
    bad[2] = 2
    assert L.mgs_mesh_build_mips(3, bad, 0x1000, total, None) == -1 and b"levels" in msg()
    resolve = lambda **kw: L.mgs_mesh_resolve_textured(*[
        {**dict(C=1, V=3, vc=0x100, F=1, faces=0x200, vcol=None, fcol=None, Ks=0x300, W=64, H=64, light=0, ambient=0.3, ws=0x1000,
                nbytes=1 << 30, rgb=0x400, depth=0x500, ids=0x600, normals=None, uvs=0x700, ft=0x800, T=3, desc=0x900, tex=0xA00,
                count=total, filt=1, stream=None), **kw}[k]
        for k in ("C", "V", "vc", "F", "faces", "vcol", "fcol", "Ks", "W", "H", "light", "ambient", "ws", "nbytes", "rgb", "depth",
                  "ids", "normals", "uvs", "ft", "T", "desc", "tex", "count", "filt", "stream")])
    assert resolve(uvs=None) == -1 and b"null" in msg()
    assert resolve(tex=None) == -1 and b"null" in msg()
    assert resolve(filt=2) == -1 and b"filter" in msg()
    assert resolve(T=0) == -1 and b"n_textures" in msg()
    assert resolve(T=4097) == -1 and b"4096" in msg()
    assert resolve(count=0) == -1 and b"texel_count" in msg()
    assert resolve(count=2 ** 31) == -1 and b"texel_count" in msg()
    assert resolve(rgb=None) == -1 and b"output" in msg()
    assert resolve(W=16369) == -1 and b"16368" in msg()
    assert resolve(nbytes=100) == -1 and b"needed" in msg()
    assert resolve(ambient=2.0) == -1 and b"ambient" in msg()
    # the fused call checks everything before its first launch
    rc = L.mgs_rasterize_mesh_textured(1, 3, 0x100, None, 0, None, None, None, 0x200, 0x300, 1, 0x400, None, None, 64, 64, 0.01, 1e10,
                                       0, 0, 0.3, 0x1000, 1 << 30, 0x500, 0x600, 0x700, 0x800, None, 0x900, 0xA00, 3, 0xB00, 0xC00,
                                       total, 5, None)
    assert rc == -1 and b"filter" in msg()
    rc = L.mgs_rasterize_mesh_textured(1, 3, 0x100, None, 0, None, None, None, 0x200, 0x300, 1, 0x400, None, None, 64, 64, 0.0, 1e10,
                                       0, 0, 0.3, 0x1000, 1 << 30, 0x500, 0x600, 0x700, 0x800, None, 0x900, 0xA00, 3, 0xB00, 0xC00,
                                       total, 1, None)
    assert rc == -1 and b"near_plane" in msg()


# ---- Mesh, Texture and the loaders ----------------------------------------------------------------------------------------------
def test_texture_and_mesh_fields_validate_carry_and_merge():
    import torch
    from robosimgs_amd import Mesh, Texture
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    t = Texture(rgb, wrap_t="mirror")
    assert tuple(t.image.shape) == (2, 3, 4) and (t.image[..., 3] == 255).all() and (t.width, t.height) == (3, 2)
    assert (t.wrap_s, t.wrap_t) == ("repeat", "mirror")
    assert torch.equal(Texture(torch.from_numpy(rgb)).image, t.image)
    for bad, word in ((rgb.astype(np.float32), "uint8"), (rgb[..., :2], r"\[h,w,3\]"), (rgb[0], r"\[h,w,3\]")):
        with pytest.raises(ValueError, match=word):
            Texture(bad)
    with pytest.raises(ValueError, match="wrap_s"):
        Texture(rgb, wrap_s="border")
    v, f = np.zeros((4, 3), np.float32), np.array([[0, 1, 2], [0, 2, 3]])
    uv = np.zeros((2, 3, 2), np.float32)
    assert Mesh(v, f, None, None, None).textures is None                            # the five positional fields, as before
    m = Mesh(v, f, face_uvs=uv, face_textures=[0, -1], textures=[t])
    assert m.has_textures and m.face_textures.dtype == torch.int32 and m.to("cpu").textures[0].wrap_t == "mirror"
    with pytest.raises(ValueError, match="go together"):
        Mesh(v, f, face_uvs=uv)
    with pytest.raises(ValueError, match="face_uvs must be"):
        Mesh(v, f, face_uvs=uv[:1], face_textures=[0, 0], textures=[t])
    with pytest.raises(ValueError, match="face_textures must be"):
        Mesh(v, f, face_uvs=uv, face_textures=[0.5, 0], textures=[t])
    with pytest.raises(ValueError, match="list of Texture"):
        Mesh(v, f, face_uvs=uv, face_textures=[0, 0], textures=[rgb])
    # merge: ids offset by the textures before, untextured parts -1 with zero uvs, ids outside a part's own set stay outside
    t2 = Texture(rgb[:1], "clamp", "clamp")
    a = Mesh(v, f, face_uvs=uv + 0.25, face_textures=[0, 7], textures=[t])
    b = Mesh(v, f)
    c = Mesh(v, f, face_uvs=uv + 0.5, face_textures=[1, 0], textures=[t, t2])
    g = Mesh.merge([a, b, c])
    assert g.face_textures.tolist() == [0, -1, -1, -1, 2, 1] and len(g.textures) == 3 and g.textures[2] is t2
    assert g.face_uvs[:2].eq(0.25).all() and g.face_uvs[2:4].eq(0).all() and g.face_uvs[4:].eq(0.5).all()
    assert Mesh.merge([b, b]).textures is None


def _glb(path, json_doc, blob):
    js = json.dumps(json_doc).encode()
    js += b" " * (-len(js) % 4)
    blob += b"\0" * (-len(blob) % 4)
    body = struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(blob), 0x004E4942) + blob
    open(path, "wb").write(b"glTF" + struct.pack("<II", 2, 12 + len(body)) + body)


def _textured_glb(path, png, *, wrap=(10497, 10497), factor=None, transform=False, uri=None, tex_coord=0, extra_map=None):
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    st = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    blob = pos.tobytes() + st.tobytes() + idx.tobytes()
    views = [dict(buffer=0, byteOffset=0, byteLength=48), dict(buffer=0, byteOffset=48, byteLength=32),
             dict(buffer=0, byteOffset=80, byteLength=12), dict(buffer=0, byteOffset=92, byteLength=len(png))]
    base = dict(index=0, texCoord=tex_coord)
    if transform:
        base["extensions"] = {"KHR_texture_transform": {"scale": [2, 2]}}
    pbr = dict(baseColorTexture=base)
    if factor is not None:
        pbr["baseColorFactor"] = factor
    mat = dict(name="skin", pbrMetallicRoughness=pbr)
    if extra_map:
        mat[extra_map] = dict(index=0)
    doc = dict(asset=dict(version="2.0"), buffers=[dict(byteLength=92 + len(png))], bufferViews=views,
               accessors=[dict(bufferView=0, componentType=5126, count=4, type="VEC3"),
                          dict(bufferView=1, componentType=5126, count=4, type="VEC2"),
                          dict(bufferView=2, componentType=5123, count=6, type="SCALAR")],
               images=[dict(uri=uri) if uri else dict(bufferView=3, mimeType="image/png")],
               samplers=[dict(wrapS=wrap[0], wrapT=wrap[1])], textures=[dict(source=0, sampler=0)], materials=[mat],
               meshes=[dict(primitives=[dict(attributes=dict(POSITION=0, TEXCOORD_0=1), indices=2, material=0)])])
    _glb(path, doc, blob + png)


def test_loaders_read_textures_only_when_asked(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import io
    from robosimgs_amd import Mesh
    pixels = np.random.default_rng(3).integers(0, 256, (3, 5, 3)).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, format="PNG")
    png = buf.getvalue()
    path = str(tmp_path / "quad.glb")
    for (ws, wt), names in (((10497, 33071), ("repeat", "clamp")), ((33648, 10497), ("mirror", "repeat")), ((33071, 33648), ("clamp", "mirror"))):
        _textured_glb(path, png, wrap=(ws, wt))
        with pytest.raises(ValueError, match="textures are not read"):
            Mesh.from_glb(path)                                                     # the default is what it was
        m = Mesh.from_glb(path, textures=True)
        assert (m.textures[0].wrap_s, m.textures[0].wrap_t) == names and m.vertex_colors is None
        assert np.array_equal(m.textures[0].image.numpy()[..., :3], pixels) and (m.textures[0].image.numpy()[..., 3] == 255).all()
        assert m.face_textures.tolist() == [0, 0]
        assert m.face_uvs.tolist() == [[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]]
    _textured_glb(path, png, factor=[0.5, 0.25, 1.0, 1.0])
    m = Mesh.from_glb(path, textures=True)
    assert m.vertex_colors.tolist() == [[0.5, 0.25, 1.0]] * 4                        # baseColorFactor is the tint
    for kw, word in ((dict(transform=True), "KHR_texture_transform"), (dict(uri="skin.png"), "external URI"),
                     (dict(tex_coord=1), "texCoord set 1"), (dict(extra_map="normalTexture"), "normalTexture"),
                     (dict(extra_map="emissiveTexture"), "emissiveTexture"), (dict(extra_map="occlusionTexture"), "occlusionTexture")):
        _textured_glb(path, png, **kw)
        with pytest.raises(ValueError, match=word):
            Mesh.from_glb(path, textures=True)
    # OBJ: vt's v is flipped, and vertex 2 carries two uvs (a seam)
    Image.fromarray(pixels).save(str(tmp_path / "skin.png"))
    (tmp_path / "quad.mtl").write_text("newmtl skin\nKd 1 1 1\nmap_Kd skin.png\nnewmtl bare\nKd 1 0 0\n")
    (tmp_path / "quad.obj").write_text("mtllib quad.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvt 0.25 0.75\n"
                                       "usemtl skin\nf 1/1 2/2 3/3\nf 1/1 3/5 4/4\nusemtl bare\nf 1/1 2/2 4/4\nusemtl skin\nf 1 2 3\n")
    plain = Mesh.from_obj(str(tmp_path / "quad.obj"))
    assert plain.textures is None and plain.n_faces == 4
    m = Mesh.from_obj(str(tmp_path / "quad.obj"), textures=True)
    assert m.face_textures.tolist() == [0, 0, -1, -1] and len(m.textures) == 1
    assert np.array_equal(m.textures[0].image.numpy()[..., :3], pixels)
    assert m.face_uvs[0].tolist() == [[0, 1], [1, 1], [1, 0]] and m.face_uvs[1].tolist() == [[0, 1], [0.25, 0.25], [0, 0]]
    assert m.faces[0, 2] == m.faces[1, 1] and m.face_uvs[0, 2].tolist() != m.face_uvs[1, 1].tolist()    # the seam
    assert m.face_uvs[2:].eq(0).all() and np.array_equal(m.faces.numpy(), plain.faces.numpy())


def test_python_layer_refuses_bad_texture_arguments_before_any_launch():
    import torch
    import robosimgs_amd
    from robosimgs_amd import mesh_render as M
    assert robosimgs_amd.build_texture_set is M.build_texture_set and robosimgs_amd.TextureSet is M.TextureSet
    t = robosimgs_amd.Texture(np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(ValueError, match="GPU"):
        M.build_texture_set([t], "cpu")
    with pytest.raises(ValueError, match="non-empty list"):
        M.build_texture_set([], "cuda")
    with pytest.raises(ValueError, match="texture_filter"):
        M._filter("nearest")
    with pytest.raises(ValueError, match="TextureSet"):
        M._texture_args([t], None, None, 1, torch.device("cpu"))
