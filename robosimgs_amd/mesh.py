"""Triangle meshes: the robot and the interactive objects of a hybrid scene, as arrays.

    box = Mesh.merge([Mesh.from_glb("body.glb"), Mesh.from_glb("lid.glb")], link_ids=[-1, 0])

`Mesh` holds vertices, faces, colours and a link id per vertex (the part a vertex moves with; link l takes the transform of
Gaussian group l); it reads binary glTF and OBJ files and merges parts.  Host-side data only: this module launches nothing.
tests/mesh_ref.py states in fp64 how such a mesh is to be rasterised as the opaque foreground of a frame.

    skin = Mesh.from_glb("robot.glb", textures=True)       # TEXCOORD_0, the base-colour image, wrap modes, baseColorFactor

A mesh may carry base-colour textures: a uv per face corner, a texture index per face and a list of `Texture`
(tests/texture_ref.py states how they are sampled).
"""
from __future__ import annotations

import json
import os
import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

_GLB_JSON, _GLB_BIN = 0x4E4F534A, 0x004E4942
_GL_TYPES = {5120: "i1", 5121: "u1", 5122: "<i2", 5123: "<u2", 5125: "<u4", 5126: "<f4"}
_GL_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}


WRAP_MODES = ("repeat", "clamp", "mirror")
_GL_WRAP = {10497: "repeat", 33071: "clamp", 33648: "mirror"}


def _pil_image():
    """PIL.Image, or None where PIL is not installed (it is never required: arrays and tensors always work)."""
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


class Texture:
    """A base-colour texture: image uint8 [h,w,4] (a tensor on any device; row 0 at the top, an RGB image gets alpha 255, alpha
    is carried and ignored) and a wrap mode per axis: "repeat", "clamp" or "mirror".  Values are used as they are, byte / 255:
    no sRGB linearisation.  image: a uint8 array or tensor [h,w,3|4], or a PIL image where PIL is installed."""

    def __init__(self, image, wrap_s: str = "repeat", wrap_t: str = "repeat"):
        Image = _pil_image()
        if Image is not None and isinstance(image, Image.Image):
            image = np.array(image.convert("RGBA" if "A" in image.getbands() else "RGB"))
        img = torch.as_tensor(image)
        if img.dtype != torch.uint8:
            raise ValueError(f"a texture must be uint8, got {img.dtype}")
        if img.dim() != 3 or img.shape[2] not in (3, 4) or img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError(f"a texture must be [h,w,3] or [h,w,4] with h, w >= 1, got {list(img.shape)}")
        if img.shape[2] == 3:
            img = torch.cat([img, torch.full_like(img[..., :1], 255)], dim=2)
        for name, m in (("wrap_s", wrap_s), ("wrap_t", wrap_t)):
            if m not in WRAP_MODES:
                raise ValueError(f"{name} must be one of {WRAP_MODES}, got {m!r}")
        self.image, self.wrap_s, self.wrap_t = img.contiguous(), wrap_s, wrap_t

    @property
    def width(self) -> int:
        return int(self.image.shape[1])

    @property
    def height(self) -> int:
        return int(self.image.shape[0])

    def to(self, device) -> "Texture":
        return Texture(self.image.to(device), self.wrap_s, self.wrap_t)


@dataclass
class Mesh:
    """vertices float32 [V,3], faces int32 [F,3]; at most one of vertex_colors [V,3] / face_colors [F,3] (float32, 0..1);
    link_ids int32 [V], -1 = static (None: all static).  Textures (all three or none): face_uvs float32 [F,3,2], one uv per
    corner, origin top-left and v down; face_textures int32 [F], an index into `textures` or any value outside it for "not
    textured"; textures, a list of Texture.  Tensors on any device."""
    vertices: Tensor
    faces: Tensor
    vertex_colors: Optional[Tensor] = None
    face_colors: Optional[Tensor] = None
    link_ids: Optional[Tensor] = None
    face_uvs: Optional[Tensor] = None
    face_textures: Optional[Tensor] = None
    textures: Optional[List[Texture]] = None

    def __post_init__(self):
        self._init_geometry()
        F = self.faces.shape[0]
        given = [x is not None for x in (self.face_uvs, self.face_textures, self.textures)]
        if any(given) and not all(given):
            raise ValueError("face_uvs, face_textures and textures go together: give all three or none")
        if all(given):
            uv = torch.as_tensor(self.face_uvs, dtype=torch.float32).contiguous()
            if tuple(uv.shape) != (F, 3, 2):
                raise ValueError(f"face_uvs must be [{F},3,2], got {list(uv.shape)}")
            ft = torch.as_tensor(self.face_textures)
            if ft.dtype.is_floating_point or ft.dtype == torch.bool or tuple(ft.shape) != (F,):
                raise ValueError(f"face_textures must be an integer array [{F}], got {ft.dtype} {list(ft.shape)}")
            self.face_uvs, self.face_textures = uv, ft.to(torch.int32).contiguous()
            self.textures = list(self.textures)
            if not self.textures or not all(isinstance(t, Texture) for t in self.textures):
                raise ValueError("textures must be a non-empty list of Texture")
        devices = {t.device for t in self._tensors()}
        if len(devices) > 1:
            raise ValueError(f"the arrays of a Mesh must share a device, got {sorted(map(str, devices))}")

    def _init_geometry(self):
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

    def _tensors(self):
        own = (self.vertices, self.faces, self.vertex_colors, self.face_colors, self.link_ids, self.face_uvs, self.face_textures)
        return [t for t in own if t is not None] + [t.image for t in (self.textures or [])]

    @property
    def has_textures(self) -> bool:
        return self.textures is not None

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
        return Mesh(mv(self.vertices), mv(self.faces), mv(self.vertex_colors), mv(self.face_colors), mv(self.link_ids),
                    mv(self.face_uvs), mv(self.face_textures),
                    None if self.textures is None else [t.to(device) for t in self.textures])

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
        if not any(m.has_textures for m in meshes):
            return Mesh(verts, faces, vcol, fcol, links)
        # texture ids are offset by the textures of the parts before; an untextured part gets -1 and zero uvs
        uvs, ids, textures = [], [], []
        for m in meshes:
            if m.has_textures:
                T = len(m.textures)
                inside = (m.face_textures >= 0) & (m.face_textures < T)
                uvs.append(m.face_uvs)
                ids.append(torch.where(inside, m.face_textures + len(textures), torch.full_like(m.face_textures, -1)))
                textures += m.textures
            else:
                uvs.append(torch.zeros((m.n_faces, 3, 2), dtype=torch.float32, device=dev))
                ids.append(torch.full((m.n_faces,), -1, dtype=torch.int32, device=dev))
        return Mesh(verts, faces, vcol, fcol, links, torch.cat(uvs), torch.cat(ids), textures)

    @staticmethod
    def from_obj(path: str, textures: bool = False) -> "Mesh":
        """Wavefront OBJ, `v x y z` and `f a b c` lines only (`a/b/c` index forms and negative indices are understood; a
        polygon of more than three corners is refused).  Every other line is skipped.

        textures=True also reads `vt u v`, the uv index of every `a/b/c` corner and `mtllib` / `usemtl` with the `map_Kd` image
        of each material, looked up beside the file and decoded with PIL (an ImportError says so where PIL is missing).  OBJ's
        v points up: it is flipped at load (v' = 1 - v).  One vertex may carry different uvs in different faces (a seam): uvs
        are per corner.  A face without uv indices, or whose material has no map_Kd, is not textured (-1)."""
        if textures:
            return _obj_textured(path)
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

    def to_obj(self, path: str) -> None:
        """Wavefront OBJ: a `v x y z` line per vertex, `v x y z r g b` where the mesh has vertex_colors (the colour extension
        most viewers and simulators' importers read), and a `f a b c` line per face, 1-based.  Coordinates are written with
        nine significant digits, so Mesh.from_obj reads back the float32 values given.  Face colours, link ids and textures
        are not written.  Reads the arrays back when they are on the GPU."""
        v = self.vertices.detach().cpu().numpy()
        f = self.faces.detach().cpu().numpy().astype(np.int64) + 1
        rows = v if self.vertex_colors is None else np.concatenate([v, self.vertex_colors.detach().cpu().numpy()], 1)
        with open(path, "w", encoding="utf-8") as fh:
            fh.write(f"# {len(v)} vertices, {len(f)} faces\n")
            fh.writelines("v " + " ".join(f"{x:.9g}" for x in row) + "\n" for row in rows)
            fh.writelines(f"f {a} {b} {c}\n" for a, b, c in f)

    def sample_points(self, n: int, seed: int = 0) -> np.ndarray:
        """n points on the surface, float32 [n,3] on the host: faces drawn with probability proportional to their area, a
        uniform point in each (the square-root fold of two uniforms), from numpy.random.default_rng(seed) -- the same
        points for the same seed.  The target cloud of register_points for a scanned object or a robot link.  Reads the
        arrays back when they are on the GPU."""
        n = int(n)
        if n < 0:
            raise ValueError(f"n must not be negative, got {n}")
        v = self.vertices.detach().cpu().numpy().astype(np.float64)
        f = self.faces.detach().cpu().numpy().astype(np.int64)
        if f.shape[0] == 0:
            raise ValueError("the mesh has no face to sample")
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
        if not (np.isfinite(area).all() and area.sum() > 0):
            raise ValueError("the mesh has no finite positive area to sample")
        rng = np.random.default_rng(seed)
        face = rng.choice(f.shape[0], size=n, p=area / area.sum())
        r1, r2 = np.sqrt(rng.random(n))[:, None], rng.random(n)[:, None]
        return ((1.0 - r1) * a[face] + r1 * (1.0 - r2) * b[face] + r1 * r2 * c[face]).astype(np.float32)

    @staticmethod
    def from_glb(path: str, textures: bool = False) -> "Mesh":
        """Binary glTF 2.0: POSITION, indices (u8 / u16 / u32, or none), optional COLOR_0 (float or normalised u8 / u16; alpha
        dropped), mode TRIANGLES only; the primitives of all meshes are merged in file order.  Refused with a ValueError: a
        node that carries a transform, any other primitive mode, a material with a texture, sparse accessors and buffers
        outside the file.

        textures=True reads a material's baseColorTexture instead of refusing it: TEXCOORD_0 (as per-corner face_uvs), the
        image from the binary chunk (decoded with PIL; an ImportError says so where PIL is missing), the sampler's wrap modes,
        and baseColorFactor (times COLOR_0 where present) as the vertex-colour tint.  Still refused, each by name: a texCoord
        set other than 0, KHR_texture_transform, an image at an external URI, and metallic-roughness, normal, occlusion and
        emissive maps."""
        if textures and _pil_image() is None:
            raise ImportError("Mesh.from_glb(textures=True) decodes images with PIL (Pillow), which is not installed")
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
            if textures:
                name = mat.get("name", "?")
                other = [k for k in ("metallicRoughnessTexture",) if k in pbr] + \
                        [k for k in ("normalTexture", "occlusionTexture", "emissiveTexture") if k in mat]
                if other:
                    raise ValueError(f"{path}: material {name!r} uses {', '.join(other)}: only baseColorTexture is read")
                base = pbr.get("baseColorTexture")
                if base is not None and base.get("texCoord", 0) != 0:
                    raise ValueError(f"{path}: material {name!r} samples texCoord set {base['texCoord']}: only TEXCOORD_0 is read")
                if base is not None and "KHR_texture_transform" in base.get("extensions", {}):
                    raise ValueError(f"{path}: material {name!r} uses KHR_texture_transform: texture transforms are not read")
            elif any(k in pbr for k in ("baseColorTexture", "metallicRoughnessTexture")) or \
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

        tex_list, tex_of = [], {}                      # the Textures read so far, glTF texture index -> position in tex_list

        def texture(ti):
            if ti not in tex_of:
                tex = doc["textures"][ti]
                image = doc["images"][tex["source"]]
                if "uri" in image:
                    raise ValueError(f"{path}: image {tex['source']} lies at an external URI ({image['uri'][:40]!r}): only images "
                                     f"in the binary chunk are read")
                bv = doc["bufferViews"][image["bufferView"]]
                start, size = bv.get("byteOffset", 0), bv["byteLength"]
                if bv.get("buffer", 0) != 0 or start + size > len(blob):
                    raise ValueError(f"{path}: image {tex['source']} reaches outside the binary chunk")
                import io
                sampler = doc["samplers"][tex["sampler"]] if "sampler" in tex else {}
                wrap = [sampler.get(k, 10497) for k in ("wrapS", "wrapT")]
                if any(w not in _GL_WRAP for w in wrap):
                    raise ValueError(f"{path}: sampler wrap modes {wrap} are not glTF's 10497 / 33071 / 33648")
                tex_of[ti] = len(tex_list)
                tex_list.append(Texture(_pil_image().open(io.BytesIO(blob[start:start + size])), _GL_WRAP[wrap[0]], _GL_WRAP[wrap[1]]))
            return tex_of[ti]

        parts, part_uvs, part_ids = [], [], []
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
                tri = idx.astype(np.int64).reshape(-1, 3)
                if textures:
                    mat = doc["materials"][prim["material"]] if "material" in prim else {}
                    pbr = mat.get("pbrMetallicRoughness", {})
                    uv, tid = np.zeros((len(tri), 3, 2), np.float32), -1
                    if "baseColorTexture" in pbr and "TEXCOORD_0" in prim["attributes"]:
                        st, _ = accessor(prim["attributes"]["TEXCOORD_0"])
                        if st.shape[1] != 2 or len(st) != len(pos):
                            raise ValueError(f"{path}: TEXCOORD_0 must be VEC2, one per vertex")
                        if st.dtype.kind == "u":
                            st = st.astype(np.float32) / float(np.iinfo(st.dtype).max)
                        uv, tid = st.astype(np.float32)[tri], texture(pbr["baseColorTexture"]["index"])
                    factor = np.asarray(pbr.get("baseColorFactor", [1.0, 1.0, 1.0, 1.0]), np.float32)[:3]
                    if tid >= 0 and (col is not None or (factor != 1).any()):
                        col = (np.ones((len(pos), 3), np.float32) if col is None else col) * factor
                    part_uvs.append(uv)
                    part_ids.append(np.full(len(tri), tid, np.int32))
                parts.append(Mesh(pos.astype(np.float32), tri, vertex_colors=col))
        if not parts:
            raise ValueError(f"{path}: no mesh primitive")
        if tex_list and any(p.vertex_colors is not None for p in parts):
            # Mesh.merge gives a part without colours 0.7 grey; the tint of a textured part without colours is 1
            parts = [Mesh(p.vertices, p.faces, vertex_colors=torch.ones_like(p.vertices))
                     if p.vertex_colors is None and (ids >= 0).any() else p for p, ids in zip(parts, part_ids)]
        merged = parts[0] if len(parts) == 1 else Mesh.merge(parts)
        if not tex_list:
            return merged
        return Mesh(merged.vertices, merged.faces, merged.vertex_colors, merged.face_colors, merged.link_ids,
                    np.concatenate(part_uvs), np.concatenate(part_ids), tex_list)


def _obj_textured(path: str) -> Mesh:
    """Mesh.from_obj(path, textures=True)."""
    Image = _pil_image()
    if Image is None:
        raise ImportError("Mesh.from_obj(textures=True) decodes images with PIL (Pillow), which is not installed")
    folder = os.path.dirname(os.path.abspath(path))
    verts, vts, faces, corners, mats = [], [], [], [], []
    maps, current = {}, None                               # material name -> map_Kd file
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        for no, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                if len(parts) < 4:
                    raise ValueError(f"{path}:{no}: a vertex needs three coordinates")
                verts.append([float(parts[1]), float(parts[2]), float(parts[3])])
            elif parts[0] == "vt":
                if len(parts) < 3:
                    raise ValueError(f"{path}:{no}: a texture coordinate needs u and v")
                vts.append([float(parts[1]), 1.0 - float(parts[2])])           # OBJ's v points up
            elif parts[0] == "mtllib":
                name = None
                with open(os.path.join(folder, line.split(None, 1)[1].strip()), "r", encoding="utf-8", errors="replace") as mh:
                    for ml in mh:
                        mp = ml.split(None, 1)
                        if len(mp) == 2 and mp[0] == "newmtl":
                            name = mp[1].strip()
                        elif len(mp) == 2 and mp[0] == "map_Kd" and name is not None:
                            maps[name] = mp[1].split()[-1]
            elif parts[0] == "usemtl":
                current = line.split(None, 1)[1].strip() if len(parts) > 1 else None
            elif parts[0] == "f":
                if len(parts) != 4:
                    raise ValueError(f"{path}:{no}: only triangles are read, this face has {len(parts) - 1} corners")
                toks = [tok.split("/") for tok in parts[1:]]
                idx = [int(t[0]) for t in toks]
                faces.append([i - 1 if i > 0 else len(verts) + i for i in idx])
                uv = [int(t[1]) if len(t) > 1 and t[1] else 0 for t in toks]
                corners.append([i - 1 if i > 0 else (len(vts) + i if i < 0 else -1) for i in uv])
                mats.append(current)
    F = len(faces)
    names = [m for m in dict.fromkeys(mats) if m in maps]
    tex = [Texture(Image.open(os.path.join(folder, maps[m]))) for m in names]
    mesh = Mesh(np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3))
    if not tex:
        return mesh
    corners = np.asarray(corners, np.int64).reshape(F, 3)
    if (corners >= len(vts)).any():
        raise ValueError(f"{path}: a face names texture coordinate {int(corners.max()) + 1}, the file has {len(vts)}")
    has_uv = (corners >= 0).all(1)
    ids = np.array([names.index(m) if m in names and ok else -1 for m, ok in zip(mats, has_uv)], np.int32)
    uvs = np.zeros((F, 3, 2), np.float32)
    if len(vts):
        uvs[ids >= 0] = np.asarray(vts, np.float32)[corners[ids >= 0]]
    return Mesh(mesh.vertices, mesh.faces, face_uvs=uvs, face_textures=ids, textures=tex)


__all__ = ["Mesh", "Texture", "WRAP_MODES"]
