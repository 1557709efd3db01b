"""Time the textured mesh operator on the GPU (profiles/mesh_texture/README.md): the open box at 1920 x 1080 (`top` view) with one
2048 x 2048 texture on every face, device events around the five launches of a render.

    python scripts/mesh_texture_timing.py [--baseline-lib PATH/libmgs.so] [--calls 50] [--rounds 5]

Per round, interleaved: the untextured mgs_rasterize_mesh of this build, the same entry point of --baseline-lib (another
build of the library, e.g. the parent commit's: called through ctypes on the same buffers), the textured render with both
filters, and the mip build.  Every figure is the median over --calls calls after a warm-up; the rounds give the run-to-run
spread that the comparison with the baseline is held to.  One JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_scenes as MS          # noqa: E402
import texture_ref as TR          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--texture-side", type=int, default=2048)
    args = ap.parse_args()
    import torch
    from robosimgs_amd import Mesh, MeshRenderer, Texture, _lib, build_texture_set
    from robosimgs_amd._lib import ptr, stream_handle
    assert torch.cuda.is_available(), "this script measures on the GPU; there is no other path"
    dev, W, H = "cuda", 1920, 1080
    box = MS.openbox()
    vm, K = MS.top_1080p(box)
    verts, faces = box["verts"], box["faces"]
    uv = (2.0 * (verts[:, :2] - verts[:, :2].min(0)) / np.ptp(verts[:, :2], axis=0)).astype(np.float32)
    tex = Texture(TR.noise_checker(args.texture_side, args.texture_side, 3, cells=16))
    plain = Mesh(verts, faces).to(dev)
    skinned = Mesh(verts, faces, face_uvs=uv[faces], face_textures=np.zeros(len(faces), np.int32), textures=[tex]).to(dev)
    vmd, Kd = torch.from_numpy(vm[None].copy()).to(dev), torch.from_numpy(K[None].copy()).to(dev)
    r0 = MeshRenderer(plain, W, H, headlight=True)
    rt = {f: MeshRenderer(skinned, W, H, headlight=True, texture_filter=f) for f in ("bilinear", "trilinear")}

    def raw(L):
        """mgs_rasterize_mesh of library L on r0's buffers."""
        fn = L.mgs_rasterize_mesh
        fn.argtypes, fn.restype = _lib._MESH_SIGNATURES["mgs_rasterize_mesh"]
        o = r0.out
        a = (1, plain.n_vertices, ptr(plain.vertices), None, 0, None, None, None, ptr(vmd), ptr(Kd), plain.n_faces, ptr(plain.faces),
             None, None, W, H, 0.01, 1e10, 0, 1, 0.3, r0.workspace.data_ptr() + r0._pad, r0.workspace.numel() - r0._pad,
             ptr(r0.verts_cam), ptr(o["rgb"]), ptr(o["depth"]), ptr(o["face_ids"]), None)
        def call():
            rc = fn(*a, stream_handle())
            assert rc == 0, rc
        return call

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return round(float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3, 2)

    jobs = {"untextured_us": raw(_lib.lib())}
    if args.baseline_lib:
        jobs["baseline_untextured_us"] = raw(ctypes.CDLL(os.path.abspath(args.baseline_lib)))
    for f, r in rt.items():
        jobs[f"textured_{f}_us"] = (lambda r=r: r.render(vmd, Kd))
    ts = rt["trilinear"].textures
    L = _lib.lib()
    jobs["mip_build_us"] = lambda: _lib.check(L.mgs_mesh_build_mips(1, ts.descriptors_host.data_ptr(), ptr(ts.texels), ts.texel_count,
                                                                   stream_handle()), "mgs_mesh_build_mips")
    rounds = {k: [] for k in jobs}
    for _ in range(args.rounds):
        for k, fn in jobs.items():
            rounds[k].append(timed(fn))
    ids = rt["trilinear"].out["face_ids"]
    res = {"config": "top_1080p", "texture": f"{args.texture_side}^2", "faces": int(plain.n_faces), "covered_px": int((ids >= 0).sum()),
           "calls": args.calls, "rounds": rounds,
           "median_us": {k: float(np.median(v)) for k, v in rounds.items()},
           "spread_us": {k: round(max(v) - min(v), 2) for k, v in rounds.items()}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
