"""Generate tests/golden/mesh_openbox.npz: the triangle meshes of the reference's openbox_output/parts/{lid,body}.glb and the
silhouettes of its six GL renders openbox_output/segmentation/view_<name>.png (800 x 800), which pin the triangle rasteriser.
Data only: no reference source is read or stored.  Re-run with:
    python tests/golden/make_mesh_golden.py
Needs /root/reference and PIL; the tests that consume the .npz need neither, and no test runs this script.

Arrays: lid_vertices / body_vertices float32 [V,3] (what hinge_openbox.npz also holds; stored again so that this file stands
alone), lid_faces / body_faces uint16 [F,3], sil_names [6], sil_shape (800, 800), sil_bits uint8 [6, 80000]: np.packbits of
"the pixel differs from pixel (0, 0)" (which is white), row-major.  The cameras are camera_reference.npz's.
"""
import json
import os
import struct

import numpy as np
from PIL import Image

REF = "/root/reference/Articulation/openbox_output"
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["top", "bottom", "front", "back", "left", "right"]


def glb_arrays(path):
    """(POSITION float32 [V,3], indices [F,3]) of the single primitive of a binary glTF, as stored."""
    data = open(path, "rb").read()
    magic, _, length = struct.unpack_from("<4sII", data, 0)
    assert magic == b"glTF"
    off, chunks = 12, {}
    while off < length:
        clen, ctype = struct.unpack_from("<II", data, off)
        chunks[ctype] = data[off + 8:off + 8 + clen]
        off += 8 + clen
    gltf, blob = json.loads(chunks[0x4E4F534A]), chunks[0x004E4942]
    assert all(set(n) <= {"name", "mesh", "children"} for n in gltf.get("nodes", [])), "a node carries a transform"
    (mesh,) = gltf["meshes"]
    (prim,) = mesh["primitives"]
    assert prim.get("mode", 4) == 4

    def read(i, dtype, width):
        a = gltf["accessors"][i]
        bv = gltf["bufferViews"][a["bufferView"]]
        assert bv.get("byteStride", 0) in (0, np.dtype(dtype).itemsize * width)
        start = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
        return np.frombuffer(blob, dtype=dtype, count=width * a["count"], offset=start)

    a_idx = gltf["accessors"][prim["indices"]]
    assert a_idx["componentType"] == 5125 and a_idx["type"] == "SCALAR"
    pos = read(prim["attributes"]["POSITION"], "<f4", 3).reshape(-1, 3)
    idx = read(prim["indices"], "<u4", 1).reshape(-1, 3)
    assert idx.max() < len(pos) <= 65536
    return np.ascontiguousarray(pos, dtype=np.float32), idx.astype(np.uint16)


out = {}
for part in ("lid", "body"):
    out[f"{part}_vertices"], out[f"{part}_faces"] = glb_arrays(os.path.join(REF, "parts", f"{part}.glb"))
hinge = np.load(os.path.join(HERE, "hinge_openbox.npz"))
assert np.array_equal(hinge["lid"], out["lid_vertices"]) and np.array_equal(hinge["body"], out["body_vertices"])
bits = []
for name in NAMES:
    img = np.asarray(Image.open(os.path.join(REF, "segmentation", f"view_{name}.png")).convert("RGB"))
    assert img.shape == (800, 800, 3) and (img[0, 0] == 255).all()
    bits.append(np.packbits((img != img[0, 0]).any(-1).reshape(-1)))
out["sil_names"], out["sil_shape"], out["sil_bits"] = np.array(NAMES), np.array([800, 800]), np.stack(bits)
path = os.path.join(HERE, "mesh_openbox.npz")
np.savez_compressed(path, **out)
print("wrote mesh_openbox.npz:", {k: getattr(v, "shape", None) for k, v in out.items()}, os.path.getsize(path), "bytes")
