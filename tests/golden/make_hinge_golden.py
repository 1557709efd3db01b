"""Generate tests/golden/hinge_openbox.npz: the fp32 vertex arrays of the reference's openbox_output/parts/{lid,body}.glb
and the hinge block of its openbox_output/urdf/metadata.json (what its hinge detector recorded for those two meshes).
Data only: no reference source is read or stored.  Re-run with:
    python tests/golden/make_hinge_golden.py
Needs /root/reference; the tests that consume the .npz do not, and no test runs this script.
"""
import json
import os
import struct

import numpy as np

REF = "/root/reference/Articulation/openbox_output"
HERE = os.path.dirname(os.path.abspath(__file__))


def glb_vertices(path):
    """POSITION of every primitive of a binary glTF, in file order, as stored (float32; these files carry no node transform)."""
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
    out = []
    for mesh in gltf["meshes"]:
        for prim in mesh["primitives"]:
            a = gltf["accessors"][prim["attributes"]["POSITION"]]
            bv = gltf["bufferViews"][a["bufferView"]]
            assert a["componentType"] == 5126 and a["type"] == "VEC3" and bv.get("byteStride", 12) == 12
            start = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
            out.append(np.frombuffer(blob, dtype="<f4", count=3 * a["count"], offset=start).reshape(-1, 3))
    return np.ascontiguousarray(np.concatenate(out), dtype=np.float32)


hinge = json.load(open(os.path.join(REF, "urdf", "metadata.json")))["hinge"]
out = {"lid": glb_vertices(os.path.join(REF, "parts", "lid.glb")), "body": glb_vertices(os.path.join(REF, "parts", "body.glb")),
       "position": np.array(hinge["original_position"], dtype=np.float64), "axis": np.array(hinge["axis"], dtype=np.float64),
       "axis_confidence": np.float64(hinge["axis_confidence"]),
       "translation_applied": np.array(hinge["translation_applied"], dtype=np.float64), "threshold": np.float64(0.01)}
np.savez_compressed(os.path.join(HERE, "hinge_openbox.npz"), **out)
print("wrote hinge_openbox.npz:", {k: getattr(v, "shape", None) for k, v in out.items()})
