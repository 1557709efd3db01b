"""Data-generation loop for a hybrid scene (the frames RoboSimGS is built for): a static 3DGS background from an unchanged
FrameRenderer, and in front of it a triangle mesh -- the reference's open box, its lid on a hinge -- rendered by
MeshRenderer and composited by depth.  The loop of examples/articulated_scene.py with the stand-in disc replaced by a
mesh render.  Synthetic background, so it runs anywhere an MI355X is visible:

    python examples/hybrid_scene.py [n_frames] [--exact] [--textured] [--lens k1,k2,p1,p2,k3]

The mesh render and the composite run eagerly on the consumer stream, once per fetched frame: there is no graph around
them (composite_over builds its backdrop tensor from a host list and allocates its outputs on every call, so it is not
capture-safe; and DESIGN.md 4.16 says why mesh kernels stay out of FrameRenderer's graphs).

--exact renders the background eagerly through rasterization(foreground=...) instead and writes its hybrid_rgb: every
pixel's own front-to-back blend stopped at the mesh's depth, where composite_over compares the mesh with
the frame's expected depth once.  No FrameRenderer and no graph on that path.

--textured gives the box a procedural base-colour texture generated here (planks and a coarse checker, 512 x 512, no asset
file) with planar uvs per face; MeshRenderer packs it and builds its mipmaps once, and render() filters it trilinearly
(DESIGN.md 4.18).

--lens k1,k2,p1,p2,k3 renders BOTH layers under one OpenCV pinhole lens (cv2.calibrateCamera's distCoeffs): the Gaussians
through pinhole_distortion= and the mesh at each pixel's own ray solved from the same lens, so the box
sits on the background it was placed in, as in a raw, un-resampled capture.  With --exact too.  Not with --textured.
"""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from robosimgs_amd import (FrameRenderer, Mesh, MeshRenderer, Texture, camera_ring, composite_over,  # noqa: E402
                           frame_to_u8, rasterization, synthetic_scene)
from robosimgs_amd.articulation import Hinge  # noqa: E402


def open_box():
    """(Mesh with the lid as link 0, Hinge) from the reference's own open box (tests/golden)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_openbox.npz"))
    h = np.load(os.path.join(ROOT, "tests", "golden", "hinge_openbox.npz"))
    grey = lambda n, v: torch.full((n, 3), v)
    lid = Mesh(g["lid_vertices"], g["lid_faces"].astype(np.int64), vertex_colors=grey(len(g["lid_vertices"]), 0.9) * torch.tensor([1.0, 0.45, 0.2]))
    body = Mesh(g["body_vertices"], g["body_faces"].astype(np.int64), vertex_colors=grey(len(g["body_vertices"]), 0.8))
    joint = np.zeros(16)
    joint[0:3], joint[3:6] = h["position"], h["axis"]
    return Mesh.merge([lid, body], link_ids=[0, -1]), Hinge(torch.from_numpy(joint))


def procedural_texture(side=512):
    """uint8 [side,side,3]: wooden planks (a slow sine grain per plank) under a coarse checker."""
    y, x = np.mgrid[0:side, 0:side] / side
    plank = np.floor(x * 8)
    grain = 0.5 + 0.5 * np.sin(2 * np.pi * (y * 3 + 0.37 * plank) + 6 * np.sin(2 * np.pi * x * 8))
    base = np.stack([0.55 + 0.25 * grain, 0.36 + 0.18 * grain, 0.2 + 0.1 * grain], -1)
    check = ((np.floor(x * 4) + np.floor(y * 4)) % 2)[..., None]
    return np.clip(np.round(255 * base * (0.8 + 0.2 * check)), 0, 255).astype(np.uint8)


def textured(box):
    """`box` with planar uvs (the two longer axes of its bounding box, two repeats across) and one texture on every face."""
    v = box.vertices.numpy()
    axes = np.argsort(np.ptp(v, axis=0))[1:]
    uv = (2.0 * (v[:, axes] - v[:, axes].min(0)) / np.ptp(v[:, axes], axis=0)).astype(np.float32)
    faces = box.faces.numpy()
    return Mesh(box.vertices, box.faces, box.vertex_colors, box.face_colors, box.link_ids, uv[faces],
                np.zeros(len(faces), np.int32), [Texture(procedural_texture(), "repeat", "mirror")])


def main():
    flags = ("--exact", "--textured")
    argv = [a for a in sys.argv[1:] if a not in flags]
    lens = None
    if "--lens" in argv:
        at = argv.index("--lens")
        lens = tuple(float(v) for v in argv[at + 1].split(","))
        del argv[at:at + 2]
    lens_kw = {} if lens is None else {"pinhole_distortion": lens}
    exact = "--exact" in sys.argv[1:]
    n_frames = int(argv[0]) if argv else 60
    W, H = 1280, 720
    scene = synthetic_scene(300_000, math.log(0.02), 3, seed=0)
    cams = camera_ring(n_frames, W, H, radius=7.0)
    r = None if exact else FrameRenderer(scene.to_torch("cuda", 3), W, H, render_mode="RGB+ED", frames_in_flight=3,
                      sizing_camera=(cams[0].viewmat(), cams[0].K), capacity_margin=2.0, **lens_kw)
    box, hinge = open_box()
    if "--textured" in sys.argv[1:]:
        box = textured(box)                                              # the vertex colours stay on as the tint
    mesh = MeshRenderer(box.to("cuda"), W, H, headlight=True, **lens_kw)            # workspace and outputs allocated once
    # per frame: the camera and the lid's pose, uploaded before the loop so that the loop itself copies nothing
    angles = 0.6 * (1.0 - np.cos(2 * np.pi * np.arange(n_frames) / n_frames)) / 2
    R, t = hinge.pose(angles)                                            # [n,3,3], [n,3]
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda")
    R_dev, t_dev = to_dev(R)[:, None].contiguous(), to_dev(t)[:, None].contiguous()      # [n,1,3,3], [n,1,3]: one link
    vm_dev = to_dev(np.stack([c.viewmat() for c in cams]))[:, None].contiguous()
    K_dev = to_dev(np.stack([c.K for c in cams]))[:, None].contiguous()

    frames, box_pixels = [], []

    def consume(i, f):
        fg_rgb, fg_depth, meta = mesh.render(vm_dev[i], K_dev[i], rotations=R_dev[i], translations=t_dev[i])
        rgb, depth = composite_over(f["colors"][..., :3], f["alphas"], f["colors"][..., 3], fg_rgb[0], fg_depth[0],
                                    backdrop=(0.05, 0.05, 0.08))
        frames.append(frame_to_u8(rgb, torch.ones(H, W, device="cuda")).cpu())     # already composited: alpha 1
        box_pixels.append((meta["face_ids"] >= 0).sum())

    def consume_exact(i, t):
        fg_rgb, fg_depth, meta = mesh.render(vm_dev[i], K_dev[i], rotations=R_dev[i], translations=t_dev[i])
        _, _, m = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vm_dev[i], K_dev[i], W, H,
                                sh_degree=t["sh_degree"], render_mode="RGB+ED", foreground=(fg_rgb, fg_depth),
                                backdrop=(0.05, 0.05, 0.08), **lens_kw)
        frames.append(frame_to_u8(m["hybrid_rgb"][0], torch.ones(H, W, device="cuda")).cpu())
        box_pixels.append((meta["face_ids"] >= 0).sum())

    tickets, nxt = [], 0
    scene_t = scene.to_torch("cuda", 3) if exact else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_frames if exact else 0):
        consume_exact(i, scene_t)
    for i in range(0 if exact else n_frames):
        while nxt < n_frames and len(tickets) < r.n_slots:
            tickets.append(r.submit(cams[nxt].viewmat(), cams[nxt].K))
            nxt += 1
        tk = tickets.pop(0)
        consume(i, r.fetch(tk))
        r.release(tk)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{n_frames} frames of {W}x{H}, {box.n_faces} mesh faces in front of {len(scene)} Gaussians: "
          f"{n_frames / dt:.0f} frames/s including the mesh render, "
          f"{'the exact composite (eager)' if exact else 'compositing'}, 8-bit conversion and download")
    print("mean pixel value of the first / last frame:", float(frames[0].float().mean()), float(frames[-1].float().mean()))
    print("pixels of the box in the first / middle frame:", int(box_pixels[0]), int(box_pixels[n_frames // 2]))
    if lens is not None:
        print("both layers under the lens", lens)


if __name__ == "__main__":
    main()
