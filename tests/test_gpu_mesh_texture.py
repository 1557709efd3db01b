"""Textured meshes on the GPU (include/mgs_mesh_texture.h, csrc/mesh_texture.hip, robosimgs_amd/mesh_render.py) against the
fp64 statement of tests/texture_ref.py: the mip chains bit for bit; the random scenes with three textures, every wrap mode
and both filters inside the counted bound, with the raster outputs bit-equal to the untextured operator's; a mixed mesh;
meshes without textures and with no textured face, bit-identical to the existing entry point; the closed-form quads; the
hostile inputs (tests/test_mesh_texture_host.py runs the same code under a sanitizer on the host); two cameras; a repeated
call; MeshRenderer on the textured open box."""
import numpy as np
import pytest
import torch

import mesh_ref as MR
import mesh_scenes as MS
import texture_ref as TR
import texture_scenes as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILTERS = ["bilinear", "trilinear"]
WRAPS = [(TR.REPEAT, TR.CLAMP, TR.MIRROR), (TR.CLAMP, TR.MIRROR, TR.REPEAT), (TR.MIRROR, TR.REPEAT, TR.CLAMP)]
EYE = np.eye(4, dtype=np.float32)


def _textures(tex):
    from robosimgs_amd import Texture
    return [Texture(image, ws, wt) for image, ws, wt in tex]


def _mesh(c, tex=None, **kw):
    from robosimgs_amd import Mesh
    if tex is not None:
        kw.update(face_uvs=c["face_uvs"], face_textures=c["face_textures"], textures=_textures(tex))
    return Mesh(c["verts"], c["faces"], **kw).to(DEV)


def _render(mesh, K, W, H, **kw):
    from robosimgs_amd import rasterize_mesh
    rgb, depth, meta = rasterize_mesh(mesh, EYE, K, W, H, return_normals=True, **kw)
    return dict(rgb=rgb[0].cpu().numpy(), depth=depth[0].cpu().numpy(), face_ids=meta["face_ids"][0].cpu().numpy(),
                normals=meta["normals"][0].cpu().numpy())


def _same_bits(a, b, keys=("rgb", "depth", "face_ids", "normals")):
    for k in keys:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


@pytest.mark.parametrize("size", TS.MIP_SIZES)
def test_mip_chains_are_bit_equal_to_the_statement(size):
    from robosimgs_amd import Texture, build_texture_set
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    images = [rng.integers(0, 256, (h, w, 4)).astype(np.uint8), rng.integers(0, 256, (3, 2, 3)).astype(np.uint8)]
    ts = build_texture_set([Texture(im) for im in images], DEV)
    for t, im in enumerate(images):
        chain = TR.mip_chain(im)
        assert int(ts.descriptors_host[t, 2]) == len(chain)
        for l, level in enumerate(chain):
            assert np.array_equal(ts.level(t, l).cpu().numpy(), level), (t, l)
    assert ts.texel_count == sum(lv.shape[0] * lv.shape[1] for im in images for lv in TR.mip_chain(im))
    assert torch.equal(ts.descriptors.cpu(), ts.descriptors_host)


@pytest.mark.parametrize("size", [(37, 29), (64, 64)])
def test_random_scenes_stay_inside_the_counted_bound_under_every_wrap_mode_and_filter(size):
    W, H = size
    c = TR.random_textured_scene(W, H)
    R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H)
    plain = _render(_mesh(c), c["K"], W, H)
    for k, wraps in enumerate(WRAPS):
        tex = TR.scene_textures(wraps)
        for texture_filter in FILTERS:
            light = dict(headlight=True, ambient=0.25) if k == 1 else {}
            out = _render(_mesh(c, tex), c["K"], W, H, texture_filter=texture_filter, **light)
            _same_bits(out, plain, ("depth", "face_ids", "normals"))               # the raster outputs do not move
            r = R.check_raster(out["face_ids"], out["depth"])
            res = TR.check_textured_shading(R, r, c["faces"], out["rgb"], c["face_uvs"], c["face_textures"], tex, texture_filter, **light)
            assert res["textured"] >= 20 and res["over_cap"] <= TR.CAP_SHARE
            print(f"\n{W}x{H} {wraps[0]} {texture_filter}: worst rgb ratio {res['worst']:.3f}, textured {res['textured']}")


def test_mixed_mesh_untextured_faces_keep_their_bits_and_textured_ones_are_tinted():
    W = H = 64
    c = TR.random_textured_scene(W, H, untextured_every=2)
    vcol = np.random.default_rng(5).uniform(0, 1, (len(c["verts"]), 3)).astype(np.float32)
    tex = TR.scene_textures()
    R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H)
    for texture_filter in FILTERS:
        plain = _render(_mesh(c, vertex_colors=vcol), c["K"], W, H, headlight=True)
        out = _render(_mesh(c, tex, vertex_colors=vcol), c["K"], W, H, headlight=True, texture_filter=texture_filter)
        _same_bits(out, plain, ("depth", "face_ids", "normals"))
        ids = out["face_ids"]
        un = (ids >= 0) & (c["face_textures"][np.maximum(ids, 0)] < 0)
        on = (ids >= 0) & ~un
        assert un.sum() >= 20 and on.sum() >= 20
        assert np.array_equal(out["rgb"][un].view(np.int32), plain["rgb"][un].view(np.int32))
        assert np.array_equal(out["rgb"][ids < 0].view(np.int32), plain["rgb"][ids < 0].view(np.int32))
        assert (out["rgb"][on] <= plain["rgb"][on] * (1 + 1e-6)).all() and (out["rgb"][on] != plain["rgb"][on]).any()   # texel <= 1
        r = R.check_raster(ids, out["depth"])
        TR.check_textured_shading(R, r, c["faces"], out["rgb"], c["face_uvs"], c["face_textures"], tex, texture_filter,
                                  vertex_colors=vcol, headlight=True)


def test_meshes_without_textured_faces_are_bit_identical_to_the_existing_entry_point():
    from robosimgs_amd import build_texture_set, mesh_raster, mesh_resolve
    W, H = 37, 29
    c = TR.random_textured_scene(W, H)
    tex = TR.scene_textures()
    fcol = np.random.default_rng(2).uniform(0, 1, (len(c["faces"]), 3)).astype(np.float32)
    for kw in (dict(), dict(face_colors=fcol)):
        plain = _render(_mesh(c, **kw), c["K"], W, H, headlight=True)              # textures=None: the existing entry point
        none = dict(c, face_textures=np.full(len(c["faces"]), -1, np.int32))
        for texture_filter in FILTERS:
            _same_bits(_render(_mesh(none, tex, **kw), c["K"], W, H, headlight=True, texture_filter=texture_filter), plain)
    # the stage operator: textures= switches the entry point, and without it nothing changed
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
    vc, faces, K = dev(c["verts"], np.float32)[None].contiguous(), dev(c["faces"], np.int32), dev(c["K"], np.float32)[None].contiguous()
    vis, ws = mesh_raster(vc, faces, K, W, H)
    a = mesh_resolve(vc, faces, K, W, H, ws, return_normals=True)
    ts = build_texture_set(_textures(tex), DEV)
    b = mesh_resolve(vc, faces, K, W, H, ws, return_normals=True, textures=ts, face_uvs=dev(c["face_uvs"], np.float32),
                     face_textures=dev(np.full(len(c["faces"]), 9, np.int32), np.int32))
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    t = mesh_resolve(vc, faces, K, W, H, ws, textures=ts, face_uvs=dev(c["face_uvs"], np.float32),
                     face_textures=dev(c["face_textures"], np.int32), texture_filter="bilinear")
    assert not torch.equal(t["rgb"], a["rgb"]) and torch.equal(t["depth"], a["depth"])
    with pytest.raises(ValueError, match="texture_filter"):
        mesh_resolve(vc, faces, K, W, H, ws, textures=ts, face_uvs=dev(c["face_uvs"], np.float32),
                     face_textures=dev(c["face_textures"], np.int32), texture_filter="nearest")


@pytest.mark.parametrize("texture_filter", FILTERS)
def test_closed_form_quads(texture_filter):
    for c in (TS.texel_centre_case(1), TS.texel_centre_case(2)):
        out = _render(_mesh(c, c["textures"]), c["K"], c["W"], c["H"], texture_filter=texture_filter)
        assert (out["face_ids"] >= 0).all()
        R = MR.RasterRef(c["verts"], c["faces"], c["K"], c["W"], c["H"])
        r = R.check_raster(out["face_ids"], out["depth"])
        TR.check_textured_shading(R, r, c["faces"], out["rgb"], c["face_uvs"], c["face_textures"], c["textures"], texture_filter)
        if texture_filter == "trilinear" or c["textures"][0][0].shape[1] == c["W"]:
            assert np.abs(out["rgb"] - c["expect"]).max() <= 1e-5                  # the texel itself / level 1 itself
    c = TS.ramp_case()
    out = _render(_mesh(c, c["textures"]), c["K"], c["W"], c["H"], texture_filter="bilinear")
    assert np.abs(out["rgb"][c["interior"]] - c["expect"][c["interior"]][:, None]).max() <= 1e-5


def test_hostile_inputs_are_shaded_untextured_or_wrapped_as_the_statement_says():
    W, H = 37, 29
    c = TR.random_textured_scene(W, H)
    tex = TR.scene_textures()
    plain = _render(_mesh(c), c["K"], W, H, headlight=True)
    F = len(c["faces"])
    for bad_id in (3, -7, 2 ** 31 - 1):                                             # T, negative, the largest int32
        ids = np.full(F, bad_id, np.int32)
        _same_bits(_render(_mesh(dict(c, face_textures=ids), tex), c["K"], W, H, headlight=True), plain)
    for bad in (np.nan, np.inf, -np.inf):                                           # not finite: shaded untextured
        uv = c["face_uvs"].copy()
        uv[:, 1, 0] = bad
        for texture_filter in FILTERS:
            _same_bits(_render(_mesh(dict(c, face_uvs=uv), tex), c["K"], W, H, headlight=True, texture_filter=texture_filter), plain)
    R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H)
    for bad in (1e30, -1e30):                                                       # finite: wrapped
        uv = c["face_uvs"].copy()
        uv[:, 2, 1] = bad
        for texture_filter in FILTERS:
            out = _render(_mesh(dict(c, face_uvs=uv), tex), c["K"], W, H, texture_filter=texture_filter)
            r = R.check_raster(out["face_ids"], out["depth"])
            TR.check_textured_shading(R, r, c["faces"], out["rgb"], uv, c["face_textures"], tex, texture_filter)
            assert np.isfinite(out["rgb"]).all() and out["rgb"].min() >= 0 and out["rgb"].max() <= 1
    # a 1 x 1 texture alone, and a face that crosses the near plane
    near = MR.raster_cases(W, H)["crosses_near"]
    one = [(np.array([[[200, 100, 50, 7]]], np.uint8), TR.MIRROR, TR.REPEAT)]
    cn = dict(verts=near["verts"], faces=near["faces"], K=near["K"], face_uvs=np.array([[[-2, 3], [0.5, 0.5], [3, -2]]], np.float32),
              face_textures=np.zeros(1, np.int32))
    Rn = MR.RasterRef(cn["verts"], cn["faces"], cn["K"], W, H, near["near"])
    for texture_filter in FILTERS:
        out = _render(_mesh(cn, one), cn["K"], W, H, near_plane=near["near"], texture_filter=texture_filter)
        r = Rn.check_raster(out["face_ids"], out["depth"])
        res = TR.check_textured_shading(Rn, r, cn["faces"], out["rgb"], cn["face_uvs"], cn["face_textures"], one, texture_filter)
        assert res["textured"] >= 20
        assert np.abs(out["rgb"][out["face_ids"] == 0] - np.array([200, 100, 50]) / 255).max() <= 1e-6


def test_two_cameras_in_one_call_equal_two_calls_and_a_repeated_call_is_bit_identical():
    from robosimgs_amd import rasterize_mesh
    W = H = 64
    c = TR.random_textured_scene(W, H)
    mesh = _mesh(c, TR.scene_textures())
    vm = np.stack([EYE, EYE])
    vm[1, :3, :3] = MS.rotation_about([0.3, 1.0, -0.2], 0.1)
    vm[1, :3, 3] = [0.1, -0.2, 0.4]
    Ks = np.stack([c["K"], MR.pinhole(W, H, f=75.0)])
    kw = dict(headlight=True, return_normals=True)
    flat = lambda o: [o[0], o[1], o[2]["face_ids"], o[2]["normals"]]
    both = rasterize_mesh(mesh, vm, Ks, W, H, **kw)
    for k in range(2):
        one = rasterize_mesh(mesh, vm[k], Ks[k], W, H, **kw)
        for a, b in zip(flat(both), flat(one)):
            assert torch.equal(a[k].view(torch.int32), b[0].view(torch.int32)), k
    assert not torch.equal(both[0][0], both[0][1])
    again = rasterize_mesh(mesh, vm, Ks, W, H, **kw)
    for a, b in zip(flat(both), flat(again)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_mesh_renderer_on_the_textured_open_box_equals_rasterize_mesh():
    from robosimgs_amd import Mesh, MeshRenderer, Texture, rasterize_mesh
    box = MS.openbox()
    v = box["views"]["top"]
    K = MS.scaled_K(v["K"], 0.25)
    verts, faces = box["verts"], box["faces"]
    lo, span = verts.min(0), np.ptp(verts, axis=0)
    uv = ((verts - lo) / span)[:, :2].astype(np.float32) * 3.0 - 1.0               # planar uvs from x, y, past 0 .. 1: they wrap
    ids = (np.arange(len(faces)) % 3 - 1).astype(np.int32)                         # -1, 0, 1 in turn
    tex = [Texture(TR.noise_checker(64, 32, 1), "mirror", "repeat"), Texture(TR.noise_checker(5, 3, 2), "clamp", "clamp")]
    mesh = Mesh(verts, faces, link_ids=box["link_ids"], face_uvs=uv[faces], face_textures=ids, textures=tex).to(DEV)
    Rm, t = MS.lid_pose(0.6)
    for texture_filter in FILTERS:
        r = MeshRenderer(mesh, 200, 200, headlight=True, return_normals=True, texture_filter=texture_filter)
        assert r.textures.n_textures == 2 and r.textures.mipmaps
        args = dict(rotations=torch.from_numpy(Rm).to(DEV), translations=torch.from_numpy(t).to(DEV))
        rgb, depth, meta = r.render(torch.from_numpy(v["viewmat"][None]).to(DEV), torch.from_numpy(K[None]).to(DEV), **args)
        ref = rasterize_mesh(mesh, v["viewmat"], K, 200, 200, rotations=Rm, translations=t, headlight=True, return_normals=True,
                             texture_filter=texture_filter)
        for a, b in ((rgb, ref[0]), (depth, ref[1]), (meta["face_ids"], ref[2]["face_ids"]), (meta["normals"], ref[2]["normals"])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        again = r.render(torch.from_numpy(v["viewmat"][None]).to(DEV), torch.from_numpy(K[None]).to(DEV), **args)
        assert torch.equal(again[0].view(torch.int32), ref[0].view(torch.int32))
        plain = rasterize_mesh(Mesh(verts, faces, link_ids=box["link_ids"]).to(DEV), v["viewmat"], K, 200, 200, rotations=Rm,
                               translations=t, headlight=True)
        fid = meta["face_ids"][0]
        un = (fid >= 0) & (fid % 3 == 0)
        assert torch.equal(plain[2]["face_ids"], meta["face_ids"]) and un.sum() > 100 and ((fid >= 0) & ~un).sum() > 100
        assert torch.equal(rgb[0][un], plain[0][0][un]) and not torch.equal(rgb[0][(fid >= 0) & ~un], plain[0][0][(fid >= 0) & ~un])
