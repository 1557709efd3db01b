"""Hold two builds of libmgs.so to each other byte for byte on the mesh rasteriser (profiles/mesh_refactor/README.md): every
mesh entry point on the same seeded inputs, every output pre-filled with 0xA5, one build per process.

    python scripts/mesh_dump.py --lib A/libmgs.so --out a.json      # a process of its own per build
    python scripts/mesh_dump.py --out b.json                        # the tree's own build
    python scripts/mesh_dump.py --compare a.json b.json             # exit status 1 where an array differs

Entry points: mgs_rasterize_mesh, mgs_rasterize_mesh_textured (both filters, all three wrap modes), mgs_rasterize_mesh_lens
(both lens models, mild and folding) and the staged ones (mgs_mesh_vertices, mgs_mesh_lens_rays, mgs_mesh_raster[_lens],
mgs_mesh_resolve[_lens | _textured]).  Cases: tests/mesh_ref.py's raster cases at 37 x 29 and 64 x 64 (the threshold boxes
among them), the 2064 x 16 frame, the lens sizes 37 x 29, 64 x 64 and 112 x 80, the random textured scene, the open box
from `top` at 800 x 800 (the large-face list and the fixed grid) and two cameras in one call.  What is recorded per array is
its shape, its byte count and the SHA-256 of its bytes: verts_cam, the visibility field, rgb, depth, face_ids, normals and
the whole lens workspace (ray map and both tables).  The large-face list is scratch whose order the atomics decide; it is
not an output and is not recorded."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_lens_ref as ML        # noqa: E402
import mesh_ref as MR             # noqa: E402
import mesh_scenes as MS          # noqa: E402
import texture_ref as TR          # noqa: E402

SMALL = [(37, 29), (64, 64)]
LENS_SIZES = [(37, 29), (64, 64), (112, 80)]
FILTERS = ["bilinear", "trilinear"]
WRAPS = [(TR.REPEAT, TR.CLAMP, TR.MIRROR), (TR.CLAMP, TR.MIRROR, TR.REPEAT), (TR.MIRROR, TR.REPEAT, TR.CLAMP)]
EYE = np.eye(4, dtype=np.float32)


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    names = sorted(set(A) | set(B))
    bad = [n for n in names if A.get(n) != B.get(n)]
    total = sum(v["bytes"] for v in A.values())
    print(json.dumps({"arrays": len(names), "bytes": total, "differing": len(bad), "first": bad[:10]}))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libmgs.so")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    import torch
    from robosimgs_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from robosimgs_amd import (Mesh, MeshRenderer, Texture, build_texture_set, mesh_lens_rays, mesh_lens_workspace_bytes,
                               mesh_raster, mesh_resolve, mesh_vertices, mesh_workspace_bytes)
    assert torch.cuda.is_available(), "mesh_dump runs the kernels; there is no other path"
    dev = "cuda"
    record = {}

    def put(name, t):
        a = t.detach().cpu().contiguous().view(torch.uint8).numpy()
        assert name not in record, name
        record[name] = {"shape": list(t.shape), "bytes": int(a.size), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}

    def filled(shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return torch.full((n,), 0xA5, dtype=torch.uint8, device=dev).view(dtype).view(*shape)

    def outputs(C, H, W):
        return dict(rgb=filled((C, H, W, 3), torch.float32), depth=filled((C, H, W), torch.float32),
                    face_ids=filled((C, H, W), torch.int32), normals=filled((C, H, W, 3), torch.float32))

    def d(x, dtype):
        return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)

    def colours(n, seed):
        return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32)

    def lens_kw(lens):
        model, k, _ = ML.LENSES[lens]
        return dict(pinhole_distortion=k) if model == ML.BC else dict(camera_model="fisheye", distortion=k)

    def fused(name, mesh, viewmats, Ks, W, H, near=0.01, far=1e10, cull=False, links=None, **kw):
        """MeshRenderer.render: mgs_rasterize_mesh, _textured or _lens by what the mesh and kw hold."""
        C = len(viewmats)
        ws = filled((mesh_workspace_bytes(C, mesh.n_vertices, mesh.n_faces, W, H) + 256,), torch.uint8)
        r = MeshRenderer(mesh, W, H, C, near_plane=near, far_plane=far, cull_backfaces=cull, headlight=True, ambient=0.25,
                         return_normals=True, out=outputs(C, H, W), workspace=ws, **kw)
        r.verts_cam.view(torch.uint8).fill_(0xA5)
        if r.lens_workspace is not None:
            r.lens_workspace.fill_(0xA5)
        rot, tr = (None, None) if links is None else (d(links[0], np.float32), d(links[1], np.float32))
        r.render(d(viewmats, np.float32), d(Ks, np.float32), rot, tr)
        torch.cuda.synchronize()
        put(name + "/verts_cam", r.verts_cam)
        put(name + "/visibility", r.workspace[r._pad:r._pad + 8 * C * H * W])
        for k, v in r.out.items():
            put(f"{name}/{k}", v)
        if r.lens_workspace is not None:
            put(name + "/lens_workspace", r.lens_workspace[r._lens_pad:r._lens_pad + mesh_lens_workspace_bytes(C, W, H)])

    def staged(name, verts, faces, viewmats, Ks, W, H, near=0.01, far=1e10, cull=False, lens=None, textured=None, **shade):
        """The stage entry points, each on pre-filled buffers: vertices, (rays,) raster, resolve."""
        C, V, F = len(viewmats), len(verts), len(faces)
        vc = mesh_vertices(d(verts, np.float32), d(viewmats, np.float32), out=filled((C, V, 3), torch.float32))
        put(name + "/verts_cam", vc)
        fd, Kd = d(faces, np.int32), d(Ks, np.float32)
        m = None
        if lens is not None:
            lw = filled((mesh_lens_workspace_bytes(C, W, H) + 256,), torch.uint8)
            m = mesh_lens_rays(Kd, W, H, workspace=lw, **lens_kw(lens))
            put(name + "/lens_workspace", m.workspace[m.pad:m.pad + mesh_lens_workspace_bytes(C, W, H)])
        ws = filled((mesh_workspace_bytes(C, V, F, W, H) + 256,), torch.uint8)
        vis, ws = mesh_raster(vc, fd, Kd, W, H, near_plane=near, far_plane=far, cull_backfaces=cull, workspace=ws, rays=m)
        put(name + "/visibility", vis)
        tex = {} if textured is None else dict(textures=textured[0], face_uvs=d(textured[1], np.float32),
                                                face_textures=d(textured[2], np.int32), texture_filter=textured[3])
        res = mesh_resolve(vc, fd, Kd, W, H, ws, headlight=True, ambient=0.25, return_normals=True, out=outputs(C, H, W),
                           rays=m, **{k: d(v, np.float32) for k, v in shade.items()}, **tex)
        torch.cuda.synchronize()
        for k, v in res.items():
            put(f"{name}/{k}", v)

    def textures_of(tex):
        return [Texture(image, ws, wt) for image, ws, wt in tex]

    # ---- the small cases of the host tests: pinhole, fused and staged
    for W, H in SMALL:
        for cname, c in MR.raster_cases(W, H).items():
            vcol = colours(len(c["verts"]), 5)
            mesh = Mesh(c["verts"], c["faces"], vertex_colors=vcol).to(dev)
            fused(f"pinhole/{W}x{H}/{cname}/fused", mesh, EYE[None], c["K"][None], W, H, c["near"], c["far"], c["cull"])
            staged(f"pinhole/{W}x{H}/{cname}/staged", c["verts"], c["faces"], EYE[None], c["K"][None], W, H, c["near"], c["far"],
                   c["cull"], face_colors=colours(len(c["faces"]), 6))
    c = MS.wide_case()
    fused("pinhole/2064x16/fused", Mesh(c["verts"], c["faces"]).to(dev), EYE[None], c["K"][None], c["width"], c["height"])
    c = MS.own_threshold_case()
    fused("pinhole/threshold/fused", Mesh(c["verts"], c["faces"]).to(dev), EYE[None], c["K"][None], 64, 64)
    # ---- textured: both filters, all wrap modes, fused and staged
    for W, H in SMALL:
        c = TR.random_textured_scene(W, H, untextured_every=5)
        for k, wraps in enumerate(WRAPS):
            tex = textures_of(TR.scene_textures(wraps))
            for filt in FILTERS:
                mesh = Mesh(c["verts"], c["faces"], vertex_colors=colours(len(c["verts"]), 7) if k == 1 else None,
                            face_uvs=c["face_uvs"], face_textures=c["face_textures"], textures=tex).to(dev)
                fused(f"textured/{W}x{H}/wraps{k}/{filt}/fused", mesh, EYE[None], c["K"][None], W, H, texture_filter=filt)
                staged(f"textured/{W}x{H}/wraps{k}/{filt}/staged", c["verts"], c["faces"], EYE[None], c["K"][None], W, H,
                       textured=(build_texture_set(tex, dev), c["face_uvs"], c["face_textures"], filt))
    # ---- under a lens: both models, mild and folding, fused and staged
    for lens in ML.LENSES:
        for W, H in LENS_SIZES:
            K = ML.intrinsics(lens, W, H)
            for cname, c in MR.raster_cases(W, H).items():
                mesh = Mesh(c["verts"], c["faces"], vertex_colors=colours(len(c["verts"]), 5)).to(dev)
                fused(f"lens/{lens}/{W}x{H}/{cname}/fused", mesh, EYE[None], K[None], W, H, c["near"], c["far"], c["cull"],
                      **lens_kw(lens))
                staged(f"lens/{lens}/{W}x{H}/{cname}/staged", c["verts"], c["faces"], EYE[None], K[None], W, H, c["near"], c["far"],
                       c["cull"], lens=lens, face_colors=colours(len(c["faces"]), 6))
    # ---- the open box at 800 x 800: `top` alone, then `top` and `front` in one call, the lid posed
    box = MS.openbox()
    F = len(box["faces"])
    rng = np.random.default_rng(31)
    uvs = rng.uniform(-0.5, 1.5, (F, 3, 2)).astype(np.float32)
    tids = rng.integers(-1, 3, F).astype(np.int32)
    plain = Mesh(box["verts"], box["faces"], link_ids=box["link_ids"]).to(dev)
    for cams in (("top",), ("top", "front")):
        vm = np.stack([box["views"][n]["viewmat"] for n in cams])
        Ks = np.stack([box["views"][n]["K"] for n in cams])
        tag = "top_800" if len(cams) == 1 else "two_cameras_800"
        fused(f"pinhole/{tag}/fused", plain, vm, Ks, 800, 800, links=MS.lid_pose())
        staged(f"pinhole/{tag}/staged", box["verts"], box["faces"], vm, Ks, 800, 800)
        for filt in FILTERS:
            mesh = Mesh(box["verts"], box["faces"], link_ids=box["link_ids"], face_uvs=uvs, face_textures=tids,
                        textures=textures_of(TR.scene_textures())).to(dev)
            fused(f"textured/{tag}/{filt}/fused", mesh, vm, Ks, 800, 800, texture_filter=filt, links=MS.lid_pose())
        for lens in ("bc_mild", "kb_mild"):
            fused(f"lens/{lens}/{tag}/fused", plain, vm, Ks, 800, 800, links=MS.lid_pose(), **lens_kw(lens))
            staged(f"lens/{lens}/{tag}/staged", box["verts"], box["faces"], vm, Ks, 800, 800, lens=lens)
    out = args.out or "mesh_dump.json"
    with open(out, "w") as fh:
        json.dump(record, fh, indent=0, sort_keys=True)
    print(json.dumps({"lib": _lib.LIB_PATH, "arrays": len(record), "bytes": sum(v["bytes"] for v in record.values()), "out": out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
