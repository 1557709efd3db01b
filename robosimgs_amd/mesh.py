"""Triangle meshes: the robot and the interactive objects of a hybrid scene, as arrays.

    box = Mesh.merge([Mesh.from_glb("body.glb"), Mesh.from_glb("lid.glb")], link_ids=[-1, 0])

`Mesh` holds vertices, faces, colours and a link id per vertex (the part a vertex moves with; link l takes the transform of
Gaussian group l); it reads binary glTF and OBJ files and merges parts.  Host-side data only: this module launches nothing.
tests/mesh_ref.py states in fp64 how such a mesh is to be rasterised as the opaque foreground of a frame.
"""
from __future__ import annotations

import json
import struct
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

_GLB_JSON, _GLB_BIN = 0x4E4F534A, 0x004E4942
_GL_TYPES = {5120: "i1", 5121: "u1", 5122: "<i2", 5123: "<u2", 5125: "<u4", 5126: "<f4"}
_GL_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}


@dataclass
class Mesh:
    """vertices float32 [V,3], faces int32 [F,3]; at most one of vertex_colors [V,3] / face_colors [F,3] (float32, 0..1);
    link_ids int32 [V], -1 = static (None: all static).  Tensors on any device."""
    vertices: Tensor
    faces: Tensor
    vertex_colors: Optional[Tensor] = None
    face_colors: Optional[Tensor] = None
    link_ids: Optional[Tensor] = None

    def __post_init__(self):
        self.vertices = torch.as_tensor(self.vertices, dtype=torch.float32).contiguous()
        self.faces = torch.as_tensor(self.faces)
        if self.faces.dtype.is_floating_point or self.faces.dtype == torch.bool:
            raise ValueError(f"faces must be an integer array, got {self.faces.dtype}")
        self.faces = self.faces.to(torch.int32).contiguous()
        if self.vertices.dim() != 2 or self.vertices.shape[1] != 3:
            raise ValueError(f"vertices must be [V,3], got {list(self.vertices.shape)}")
        if self.faces.dim() != 2 or self.faces.shape[1] != 3:
            raise ValueError(f"faces must be [F,3], got {list(self.faces.shape)}")
        V, F = self.vertices.shape[0], self.faces.shape[0]
        if self.vertex_colors is not None and self.face_colors is not None:
            raise ValueError("give vertex_colors or face_colors, not both")
        for name, rows in (("vertex_colors", V), ("face_colors", F)):
            c = getattr(self, name)
            if c is not None:
                c = torch.as_tensor(c, dtype=torch.float32).contiguous()
                if tuple(c.shape) != (rows, 3):
                    raise ValueError(f"{name} must be [{rows},3], got {list(c.shape)}")
                setattr(self, name, c)
        if self.link_ids is not None:
            l = torch.as_tensor(self.link_ids)
            if l.dtype.is_floating_point or tuple(l.shape) != (V,):
                raise ValueError(f"link_ids must be an integer array [{V}], got {l.dtype} {list(l.shape)}")
            self.link_ids = l.to(torch.int32).contiguous()
        devices = {t.device for t in self._tensors()}
        if len(devices) > 1:
            raise ValueError(f"the arrays of a Mesh must share a device, got {sorted(map(str, devices))}")

    def _tensors(self):
        return [t for t in (self.vertices, self.faces, self.vertex_colors, self.face_colors, self.link_ids) if t is not None]

    @property
    def n_vertices(self) -> int:
        return int(self.vertices.shape[0])

    @property
    def n_faces(self) -> int:
        return int(self.faces.shape[0])

    @property
    def device(self):
        return self.vertices.device

    def n_links(self) -> int:
        """1 + the largest link id (0 for a static mesh).  Reads link_ids back when they are on the GPU."""
        if self.link_ids is None or self.link_ids.numel() == 0:
            return 0
        return max(0, int(self.link_ids.max().item()) + 1)

    def to(self, device) -> "Mesh":
        mv = lambda t: None if t is None else t.to(device)
        return Mesh(mv(self.vertices), mv(self.faces), mv(self.vertex_colors), mv(self.face_colors), mv(self.link_ids))

    @staticmethod
    def merge(meshes: Sequence["Mesh"], link_ids: Optional[Sequence[int]] = None) -> "Mesh":
        """One mesh of several: vertices concatenated, faces re-indexed.  link_ids: one link per part (-1 static), which
        replaces the parts' own; None keeps them (a part without any is static).  Colours survive if every part has the
        same kind; a part without colours gets 0.7 grey once any other part has them."""
        meshes = list(meshes)
        if not meshes:
            raise ValueError("Mesh.merge needs at least one mesh")
        if link_ids is not None and len(link_ids) != len(meshes):
            raise ValueError(f"link_ids names {len(link_ids)} parts, {len(meshes)} meshes were given")
        dev = meshes[0].device
        if any(m.device != dev for m in meshes):
            raise ValueError("the meshes to merge must share a device")
        offs = np.cumsum([0] + [m.n_vertices for m in meshes])
        verts = torch.cat([m.vertices for m in meshes])
        faces = torch.cat([m.faces + int(o) for m, o in zip(meshes, offs)])
        if link_ids is not None:
            links = torch.cat([torch.full((m.n_vertices,), int(l), dtype=torch.int32, device=dev) for m, l in zip(meshes, link_ids)])
        elif any(m.link_ids is not None for m in meshes):
            links = torch.cat([m.link_ids if m.link_ids is not None else torch.full((m.n_vertices,), -1, dtype=torch.int32, device=dev)
                               for m in meshes])
        else:
            links = None
        vcol = fcol = None
        has_v, has_f = [m.vertex_colors is not None for m in meshes], [m.face_colors is not None for m in meshes]
        if any(has_v) and any(has_f):
            raise ValueError("cannot merge a mesh with vertex colours and one with face colours")
        grey = lambda rows: torch.full((rows, 3), 0.7, dtype=torch.float32, device=dev)
        if any(has_v):
            vcol = torch.cat([m.vertex_colors if m.vertex_colors is not None else grey(m.n_vertices) for m in meshes])
        if any(has_f):
            fcol = torch.cat([m.face_colors if m.face_colors is not None else grey(m.n_faces) for m in meshes])
        return Mesh(verts, faces, vcol, fcol, links)

    @staticmethod
    def from_obj(path: str) -> "Mesh":
        """Wavefront OBJ, `v x y z` and `f a b c` lines only (`a/b/c` index forms and negative indices are understood; a
        polygon of more than three corners is refused).  Every other line is skipped."""
        verts, faces = [], []
        with open(path, "r", encoding="utf-8", errors="replace") as fh:
            for no, line in enumerate(fh, 1):
                parts = line.split()
                if not parts:
                    continue
                if parts[0] == "v":
                    if len(parts) < 4:
                        raise ValueError(f"{path}:{no}: a vertex needs three coordinates")
                    verts.append([float(parts[1]), float(parts[2]), float(parts[3])])
                elif parts[0] == "f":
                    if len(parts) != 4:
                        raise ValueError(f"{path}:{no}: only triangles are read, this face has {len(parts) - 1} corners")
                    idx = [int(tok.split("/")[0]) for tok in parts[1:]]
                    faces.append([i - 1 if i > 0 else len(verts) + i for i in idx])
        return Mesh(np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3))

    @staticmethod
    def from_glb(path: str) -> "Mesh":
        """Binary glTF 2.0: POSITION, indices (u8 / u16 / u32, or none), optional COLOR_0 (float or normalised u8 / u16; alpha
        dropped), mode TRIANGLES only; the primitives of all meshes are merged in file order.  Refused with a ValueError: a
        node that carries a transform, any other primitive mode, a material with a texture, sparse accessors and buffers
        outside the file."""
        data = open(path, "rb").read()
        if len(data) < 20 or data[:4] != b"glTF":
            raise ValueError(f"{path}: not a binary glTF file")
        version, length = struct.unpack_from("<II", data, 4)
        if version != 2:
            raise ValueError(f"{path}: glTF container version {version}, only 2 is read")
        off, chunks = 12, {}
        while off + 8 <= min(length, len(data)):
            clen, ctype = struct.unpack_from("<II", data, off)
            chunks.setdefault(ctype, data[off + 8:off + 8 + clen])
            off += 8 + clen + (-clen % 4)
        if _GLB_JSON not in chunks:
            raise ValueError(f"{path}: no JSON chunk")
        doc, blob = json.loads(chunks[_GLB_JSON].decode("utf-8")), chunks.get(_GLB_BIN, b"")
        for node in doc.get("nodes", []):
            moved = [k for k in ("matrix", "translation", "rotation", "scale") if k in node]
            if moved:
                raise ValueError(f"{path}: node {node.get('name', '?')!r} carries a transform ({', '.join(moved)}): not read")
        for mat in doc.get("materials", []):
            pbr = mat.get("pbrMetallicRoughness", {})
            if any(k in pbr for k in ("baseColorTexture", "metallicRoughnessTexture")) or \
                    any(k in mat for k in ("normalTexture", "occlusionTexture", "emissiveTexture")):
                raise ValueError(f"{path}: material {mat.get('name', '?')!r} uses a texture: textures are not read")
        for buf in doc.get("buffers", [])[:1]:
            if "uri" in buf:
                raise ValueError(f"{path}: the buffer lies outside the file ({buf['uri'][:40]!r})")

        def accessor(i):
            a = doc["accessors"][i]
            if "sparse" in a or "bufferView" not in a:
                raise ValueError(f"{path}: sparse accessors are not read")
            bv = doc["bufferViews"][a["bufferView"]]
            if bv.get("buffer", 0) != 0:
                raise ValueError(f"{path}: only the file's own buffer is read")
            dt, width = np.dtype(_GL_TYPES[a["componentType"]]), _GL_WIDTH[a["type"]]
            start, count = bv.get("byteOffset", 0) + a.get("byteOffset", 0), a["count"]
            stride = bv.get("byteStride", 0) or dt.itemsize * width
            if start + (count - 1) * stride + dt.itemsize * width > len(blob) if count else False:
                raise ValueError(f"{path}: accessor {i} reaches past the binary chunk")
            arr = np.ndarray((count, width), dt, blob, start, (stride, dt.itemsize))
            return np.ascontiguousarray(arr), bool(a.get("normalized", False))

        parts = []
        for mesh in doc.get("meshes", []):
            for prim in mesh.get("primitives", []):
                if prim.get("mode", 4) != 4:
                    raise ValueError(f"{path}: primitive mode {prim['mode']} is not read, only 4 (TRIANGLES)")
                if "POSITION" not in prim.get("attributes", {}):
                    raise ValueError(f"{path}: a primitive has no POSITION")
                pos, _ = accessor(prim["attributes"]["POSITION"])
                if pos.dtype != np.dtype("<f4") or pos.shape[1] != 3:
                    raise ValueError(f"{path}: POSITION must be float VEC3")
                if "indices" in prim:
                    idx, _ = accessor(prim["indices"])
                    if idx.dtype.kind != "u" or idx.shape[1] != 1:
                        raise ValueError(f"{path}: indices must be unsigned scalars")
                    idx = idx.reshape(-1)
                else:
                    idx = np.arange(pos.shape[0])
                if idx.size % 3:
                    raise ValueError(f"{path}: {idx.size} indices are not a whole number of triangles")
                col = None
                if "COLOR_0" in prim["attributes"]:
                    col, normalized = accessor(prim["attributes"]["COLOR_0"])
                    if col.dtype.kind == "u":
                        col = col.astype(np.float32) / float(np.iinfo(col.dtype).max)
                    col = np.array(col[:, :3], dtype=np.float32)
                parts.append(Mesh(pos.astype(np.float32), idx.astype(np.int64).reshape(-1, 3), vertex_colors=col))
        if not parts:
            raise ValueError(f"{path}: no mesh primitive")
        return parts[0] if len(parts) == 1 else Mesh.merge(parts)


__all__ = ["Mesh"]
