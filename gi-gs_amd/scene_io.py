"""The reference's on-disk formats, so that scenes trained by either code load in the other.

    save_ply / load_ply            point_cloud.ply exactly as GaussianModel.save_ply / load_ply lay it out
                                   (scene/gaussian_model.py:397-465, 474-578): one `vertex` element of float32
                                   properties x y z, f_dc_*, f_rest_* (channel-major, i.e. the [P,K,3] features
                                   transposed to [P,3,K]), opacity, normal_0..2, albedo_0..2, roughness, metallic,
                                   scale_*, rot_*; binary little-endian as plyfile writes by default
    save_checkpoint / load_checkpoint   chkpntN.pth = {"gaussians": GaussianModel.capture() 18-tuple, "cubemap":
                                   state_dict, "light_optimizer": state_dict, "iteration"} (train.py:466-490,
                                   scene/gaussian_model.py:82-176)
    save_mesh_ply / read_mesh_ply  a triangle mesh with per-vertex materials (mesh.Mesh; not a reference format): position,
                                   world normal, albedo as 8-bit colour, roughness, metallic, optionally the baked occlusion,
                                   triangle index lists
    save_mesh_obj / read_mesh_obj  a textured triangle mesh as Wavefront OBJ + MTL: positions, normals, one UV per face
                                   corner, and a material that names the albedo / roughness / metallic / normal / ORM images

Pure host code (numpy / torch serialization): no kernels, works on CPU tensors.  `plyfile` is not needed; the reader
parses the PLY header itself (ascii and binary little-endian vertex elements with scalar properties).  Checkpoints are
read with `torch.load(..., weights_only=True)`: nothing in the file is executed.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

NAMES = ["xyz", "f_dc", "f_rest", "opacity", "normal", "albedo", "roughness", "metallic", "scaling", "rotation"]

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def attribute_names(n_dc: int, n_rest: int, n_scale: int = 3, n_rot: int = 4):
    """GaussianModel.construct_list_of_attributes (scene/gaussian_model.py:397-416)."""
    names = ["x", "y", "z"]
    names += [f"f_dc_{i}" for i in range(n_dc)]
    names += [f"f_rest_{i}" for i in range(n_rest)]
    names.append("opacity")
    names += [f"normal_{i}" for i in range(3)]
    names += [f"albedo_{i}" for i in range(3)]
    names += ["roughness", "metallic"]
    names += [f"scale_{i}" for i in range(n_scale)]
    names += [f"rot_{i}" for i in range(n_rot)]
    return names


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def save_ply(path: str, params: Dict[str, torch.Tensor]) -> None:
    """params: the ten raw (pre-activation) tensors by group name; f_dc [P,1,3], f_rest [P,K,3]."""
    xyz = _np(params["xyz"]).astype(np.float32)
    P = xyz.shape[0]
    f_dc = np.ascontiguousarray(_np(params["f_dc"]).transpose(0, 2, 1).reshape(P, -1), dtype=np.float32)
    f_rest = np.ascontiguousarray(_np(params["f_rest"]).transpose(0, 2, 1).reshape(P, -1), dtype=np.float32)
    cols = [xyz, f_dc, f_rest, _np(params["opacity"]).reshape(P, 1), _np(params["normal"]).reshape(P, 3),
            _np(params["albedo"]).reshape(P, 3), _np(params["roughness"]).reshape(P, 1),
            _np(params["metallic"]).reshape(P, 1), _np(params["scaling"]).reshape(P, -1),
            _np(params["rotation"]).reshape(P, -1)]
    table = np.ascontiguousarray(np.concatenate([c.astype(np.float32) for c in cols], axis=1), dtype="<f4")
    names = attribute_names(f_dc.shape[1], f_rest.shape[1], cols[8].shape[1], cols[9].shape[1])
    assert table.shape[1] == len(names)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {P}"]
    header += [f"property float {n}" for n in names]
    header.append("end_header")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(table.tobytes())


def read_ply_vertices(path: str) -> Dict[str, np.ndarray]:
    """-> {property name: array [P]} of the `vertex` element (scalar properties only)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements, cur = None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                cur = {"name": tok[1], "count": int(tok[2]), "props": []}
                elements.append(cur)
            elif tok[0] == "property":
                if tok[1] == "list":
                    raise ValueError(f"{path}: list properties are not supported (element {cur['name']})")
                if tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unknown property type {tok[1]}")
                cur["props"].append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("binary_little_endian", "ascii"):
            raise ValueError(f"{path}: unsupported PLY format {fmt}")
        out = None
        for el in elements:
            dt = np.dtype([(n, "<" + t) for n, t in el["props"]])
            if fmt == "ascii":
                rows = np.loadtxt(f, max_rows=el["count"], ndmin=2) if el["count"] else np.zeros((0, len(el["props"])))
                data = {n: rows[:, i].astype(t) for i, (n, t) in enumerate(el["props"])}
            else:
                raw = f.read(dt.itemsize * el["count"])
                if len(raw) != dt.itemsize * el["count"]:
                    raise ValueError(f"{path}: truncated element {el['name']}")
                arr = np.frombuffer(raw, dtype=dt, count=el["count"])
                data = {n: arr[n] for n, _ in el["props"]}
            if el["name"] == "vertex":
                out = data
                break
        if out is None:
            raise ValueError(f"{path}: no vertex element")
        return out


def load_ply(path: str, max_sh_degree: int, device="cpu") -> Dict[str, torch.Tensor]:
    """GaussianModel.load_ply (scene/gaussian_model.py:474-578) -> the ten raw tensors by group name."""
    v = read_ply_vertices(path)

    def stack(prefix, count=None):
        names = sorted((n for n in v if n.startswith(prefix)), key=lambda s: int(s.split("_")[-1]))
        if count is not None and len(names) != count:
            raise ValueError(f"{path}: expected {count} '{prefix}*' properties, found {len(names)}")
        return np.stack([np.asarray(v[n], dtype=np.float32) for n in names], axis=1)

    P = len(v["x"])
    K = (max_sh_degree + 1) ** 2
    xyz = np.stack((v["x"], v["y"], v["z"]), axis=1).astype(np.float32)
    f_dc = stack("f_dc_", 3).reshape(P, 3, 1).transpose(0, 2, 1)
    f_rest = stack("f_rest_", 3 * K - 3).reshape(P, 3, K - 1).transpose(0, 2, 1)  # the assert at :517
    out = dict(xyz=xyz, f_dc=f_dc, f_rest=f_rest, opacity=np.asarray(v["opacity"], np.float32)[:, None],
               normal=stack("normal_", 3), albedo=stack("albedo_", 3),
               roughness=np.asarray(v["roughness"], np.float32)[:, None],
               metallic=np.asarray(v["metallic"], np.float32)[:, None], scaling=stack("scale_"), rotation=stack("rot"))
    return {k: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device) for k, a in out.items()}


_MESH_VERTEX = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"),
                ("green", "u1"), ("blue", "u1"), ("roughness", "<f4"), ("metallic", "<f4")]
_MESH_OCCLUSION = ("occlusion", "<f4")  # the optional vertex property after metallic
_MESH_IRRADIANCE = [("irradiance_r", "<f4"), ("irradiance_g", "<f4"), ("irradiance_b", "<f4")]  # the optional last three
_MESH_FACE = [("n", "u1"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")]


def save_mesh_ply(path: str, vertices, faces, normals, albedo, roughness, metallic, occlusion=None, irradiance=None) -> None:
    """A triangle mesh with its materials (mesh.Mesh's fields, tensors or arrays) as a binary little-endian PLY: vertex
    properties x y z nx ny nz (float), red green blue (uchar), roughness metallic (float); faces as `property list uchar
    int vertex_indices`.  The colour is the albedo quantised as gigs_pack_images does with bias 0.5:
    trunc(clamp(x * 255 + 0.5, 0, 255)) in float32 with the product and the sum rounded separately, NaN -> 0.
    `occlusion` ([V], mesh.bake_occlusion's; 1 = open) adds one more `property float occlusion` after metallic; with None
    the file is the one without the argument, byte for byte.  `irradiance` ([V,3], mesh.bake_light's, linear and unclamped)
    adds `property float irradiance_r / _g / _b` after that, stored as the float32 values they are; None changes nothing."""
    v = np.asarray(_np(vertices), dtype=np.float32).reshape(-1, 3)
    n = np.asarray(_np(normals), dtype=np.float32).reshape(-1, 3)
    a = np.asarray(_np(albedo), dtype=np.float32).reshape(-1, 3)
    r = np.asarray(_np(roughness), dtype=np.float32).reshape(-1)
    m = np.asarray(_np(metallic), dtype=np.float32).reshape(-1)
    f = np.asarray(_np(faces)).reshape(-1, 3)
    V = v.shape[0]
    if not (n.shape[0] == a.shape[0] == r.shape[0] == m.shape[0] == V):
        raise ValueError("save_mesh_ply: the vertex attributes must have one row per vertex")
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError("save_mesh_ply: a face refers to a vertex that does not exist")
    with np.errstate(invalid="ignore"):
        q = a * np.float32(255.0) + np.float32(0.5)
        q = np.where(np.isnan(q), np.float32(0.0), np.clip(q, np.float32(0.0), np.float32(255.0))).astype(np.uint8)
    layout = list(_MESH_VERTEX)
    if occlusion is not None:
        occlusion = np.asarray(_np(occlusion), dtype=np.float32).reshape(-1)
        if occlusion.shape[0] != V:
            raise ValueError("save_mesh_ply: occlusion must have one value per vertex")
        layout.append(_MESH_OCCLUSION)
    if irradiance is not None:
        irradiance = np.asarray(_np(irradiance), dtype=np.float32)
        if irradiance.shape != (V, 3):
            raise ValueError("save_mesh_ply: irradiance must have three values per vertex")
        layout += _MESH_IRRADIANCE
    vt = np.empty(V, dtype=layout)
    if occlusion is not None:
        vt["occlusion"] = occlusion
    if irradiance is not None:
        for i, (k, _) in enumerate(_MESH_IRRADIANCE):
            vt[k] = irradiance[:, i]
    for i, k in enumerate("xyz"):
        vt[k], vt["n" + k] = v[:, i], n[:, i]
    vt["red"], vt["green"], vt["blue"], vt["roughness"], vt["metallic"] = q[:, 0], q[:, 1], q[:, 2], r, m
    ft = np.empty(f.shape[0], dtype=_MESH_FACE)
    ft["n"] = 3
    ft["a"], ft["b"], ft["c"] = f[:, 0], f[:, 1], f[:, 2]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {V}"]
    header += ["property %s %s" % ("uchar" if t == "u1" else "float", k) for k, t in layout]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vt.tobytes())
        fh.write(ft.tobytes())


def read_mesh_ply(path: str) -> Dict[str, np.ndarray]:
    """A file of save_mesh_ply -> {vertices [V,3], faces [F,3] int32, normals [V,3], albedo [V,3] (colour / 255), roughness
    [V], metallic [V]}, and occlusion [V] if the file carries that property after metallic.  Reads these two layouts only:
    anything else raises ValueError."""
    with open(path, "rb") as f:
        lines = []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            lines.append(line.decode("ascii", "replace").strip())
            if lines[-1] == "end_header":
                break
        if len(lines) < 4 or lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
            raise ValueError(f"{path}: not a binary little-endian PLY file")
        body = [ln for ln in lines[2:-1] if ln and not ln.startswith(("comment", "obj_info"))]
        layout = list(_MESH_VERTEX)
        if len(body) > 1 + len(layout) and body[1 + len(layout)] == "property float " + _MESH_OCCLUSION[0]:
            layout.append(_MESH_OCCLUSION)
        if len(body) > 1 + len(layout) and body[1 + len(layout)] == "property float " + _MESH_IRRADIANCE[0][0]:
            layout += _MESH_IRRADIANCE
        want = ["property %s %s" % ("uchar" if t == "u1" else "float", k) for k, t in layout]
        if (len(body) != len(want) + 3 or not body[0].startswith("element vertex ") or body[1:1 + len(want)] != want
                or not body[-2].startswith("element face ") or body[-1] != "property list uchar int vertex_indices"):
            raise ValueError(f"{path}: not the mesh layout of save_mesh_ply")
        V, F = int(body[0].split()[2]), int(body[-2].split()[2])
        vdt, fdt = np.dtype(layout), np.dtype(_MESH_FACE)
        raw_v, raw_f = f.read(vdt.itemsize * V), f.read(fdt.itemsize * F)
        if len(raw_v) != vdt.itemsize * V or len(raw_f) != fdt.itemsize * F:
            raise ValueError(f"{path}: truncated")
    vt, ft = np.frombuffer(raw_v, dtype=vdt, count=V), np.frombuffer(raw_f, dtype=fdt, count=F)
    if F and not (ft["n"] == 3).all():
        raise ValueError(f"{path}: a face is not a triangle")
    faces = np.stack((ft["a"], ft["b"], ft["c"]), axis=1).astype(np.int32) if F else np.zeros((0, 3), np.int32)
    if F and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"{path}: a face refers to a vertex that does not exist")
    col = lambda *ks: np.stack([vt[k] for k in ks], axis=1).astype(np.float32)  # noqa: E731
    out = dict(vertices=col("x", "y", "z"), faces=faces, normals=col("nx", "ny", "nz"),
               albedo=col("red", "green", "blue") / np.float32(255.0), roughness=vt["roughness"].astype(np.float32),
               metallic=vt["metallic"].astype(np.float32))
    if _MESH_OCCLUSION in layout:
        out["occlusion"] = vt["occlusion"].astype(np.float32)
    if _MESH_IRRADIANCE[0] in layout:
        out["irradiance"] = col(*(k for k, _ in _MESH_IRRADIANCE))
    return out


_OBJ_MAPS = (("albedo", "map_Kd"), ("roughness", "map_Pr"), ("metallic", "map_Pm"), ("normal", "norm"), ("orm", "map_ORM"))
_OBJ_MATERIAL = "baked"


def obj_texture_names(path: str) -> Dict[str, str]:
    """The image files save_mesh_obj names by default, relative to the .obj: STEM_albedo.png, STEM_roughness.png,
    STEM_metallic.png, STEM_normal.png and STEM_orm.png (occlusion, roughness, metallic packed into one image)."""
    stem = os.path.splitext(os.path.basename(path))[0]
    return {k: "%s_%s.png" % (stem, k) for k, _ in _OBJ_MAPS}


def save_mesh_obj(path: str, vertices, faces, uvs, normals=None, textures=None) -> None:
    """A textured triangle mesh as Wavefront OBJ with its material library beside it (PATH with the extension .mtl).  The
    .obj holds `mtllib`, one `v` per vertex, one `vn` per vertex if `normals` is given, one `vt` per FACE CORNER (uvs
    [F,3,2], mesh.face_uvs'; v = 0 is the bottom row of the image), `usemtl` and `f a/ta/na` (`a/ta` without normals):
    OBJ indexes positions and UVs separately, so no vertex is split.  Floats are written with nine significant digits:
    float32 values read back exactly.  The .mtl holds one material with map_Kd (albedo), map_Pr (roughness), map_Pm
    (metallic), norm (the normal map) and map_ORM (the packed occlusion / roughness / metallic image, not a standard
    statement: readers that do not know it skip it).  `textures`: {albedo, roughness, metallic, normal, orm} -> file name
    relative to the .obj, default obj_texture_names(path).  The images themselves are the caller's to write."""
    v = np.asarray(_np(vertices), dtype=np.float32).reshape(-1, 3)
    f = np.asarray(_np(faces)).reshape(-1, 3).astype(np.int64)
    uv = np.asarray(_np(uvs), dtype=np.float32)
    if uv.shape != (f.shape[0], 3, 2):
        raise ValueError("save_mesh_obj: uvs must be [F,3,2], got %s for %d faces" % (uv.shape, f.shape[0]))
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("save_mesh_obj: a face refers to a vertex that does not exist")
    n = None
    if normals is not None:
        n = np.asarray(_np(normals), dtype=np.float32).reshape(-1, 3)
        if n.shape[0] != v.shape[0]:
            raise ValueError("save_mesh_obj: normals must have one row per vertex")
    names = dict(obj_texture_names(path))
    if textures is not None:
        if set(textures) - set(names):
            raise ValueError("save_mesh_obj: unknown texture %s" % sorted(set(textures) - set(names)))
        names.update(textures)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    mtl = os.path.splitext(path)[0] + ".mtl"
    rows = lambda tag, a: "".join("%s %s\n" % (tag, " ".join("%.9g" % x for x in r)) for r in a.tolist())  # noqa: E731
    t = 3 * np.arange(f.shape[0], dtype=np.int64)[:, None] + np.arange(3)[None] + 1
    a = f + 1
    if n is not None:
        corner = ["%d/%d/%d" % (x, y, x) for x, y in zip(a.reshape(-1).tolist(), t.reshape(-1).tolist())]
    else:
        corner = ["%d/%d" % (x, y) for x, y in zip(a.reshape(-1).tolist(), t.reshape(-1).tolist())]
    with open(path, "w", encoding="ascii") as fh:
        fh.write("mtllib %s\n" % os.path.basename(mtl))
        fh.write(rows("v", v))
        if n is not None:
            fh.write(rows("vn", n))
        fh.write(rows("vt", uv.reshape(-1, 2)))
        fh.write("usemtl %s\n" % _OBJ_MATERIAL)
        fh.write("".join("f %s %s %s\n" % tuple(corner[3 * i:3 * i + 3]) for i in range(f.shape[0])))
    with open(mtl, "w", encoding="ascii") as fh:
        fh.write("newmtl %s\nKd 1 1 1\nPr 1\nPm 1\n" % _OBJ_MATERIAL)
        fh.write("".join("%s %s\n" % (key, names[k]) for k, key in _OBJ_MAPS))


def read_mesh_obj(path: str) -> Dict:
    """A file of save_mesh_obj -> {vertices [V,3], faces [F,3] int32, vt [3F,2], uv_faces [F,3] int32 (rows of vt), uvs
    [F,3,2] = vt[uv_faces], normals [V,3] or None, mtllib, material, textures {albedo, roughness, metallic, normal, orm} ->
    the file names the .mtl gives}.  Reads what the writer writes and nothing grander: anything else raises ValueError."""
    v, vn, vt, fa, ft = [], [], [], [], []
    mtllib = material = None
    with_normals = None
    with open(path, "r", encoding="ascii") as fh:
        for line in fh:
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if tok[0] == "v" and len(tok) == 4:
                v.append([float(x) for x in tok[1:]])
            elif tok[0] == "vn" and len(tok) == 4:
                vn.append([float(x) for x in tok[1:]])
            elif tok[0] == "vt" and len(tok) == 3:
                vt.append([float(x) for x in tok[1:]])
            elif tok[0] == "f" and len(tok) == 4:
                parts = [c.split("/") for c in tok[1:]]
                if with_normals is None:
                    with_normals = len(parts[0]) == 3
                if any(len(c) != (3 if with_normals else 2) for c in parts) or (with_normals and any(c[0] != c[2] for c in parts)):
                    raise ValueError(f"{path}: not the face statement of save_mesh_obj: {line.strip()}")
                fa.append([int(c[0]) - 1 for c in parts])
                ft.append([int(c[1]) - 1 for c in parts])
            elif tok[0] == "mtllib" and len(tok) == 2:
                mtllib = tok[1]
            elif tok[0] == "usemtl" and len(tok) == 2:
                material = tok[1]
            else:
                raise ValueError(f"{path}: not a statement of save_mesh_obj: {line.strip()}")
    V, F = len(v), len(fa)
    faces = np.asarray(fa, np.int32).reshape(F, 3)
    uv_faces = np.asarray(ft, np.int32).reshape(F, 3)
    vt = np.asarray(vt, np.float32).reshape(-1, 2)
    if mtllib is None or material is None or (vn and len(vn) != V) or (F and bool(vn) != bool(with_normals)):
        raise ValueError(f"{path}: not the layout of save_mesh_obj")
    if F and (faces.min() < 0 or faces.max() >= V or uv_faces.min() < 0 or uv_faces.max() >= len(vt)):
        raise ValueError(f"{path}: a face refers to a vertex or a vt that does not exist")
    keys = {key: k for k, key in _OBJ_MAPS}
    textures, found = {}, None
    with open(os.path.join(os.path.dirname(path), mtllib), "r", encoding="ascii") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "newmtl":
                found = tok[1]
            elif tok[0] in keys and len(tok) == 2 and found == material:
                textures[keys[tok[0]]] = tok[1]
    if found != material or sorted(textures) != sorted(keys.values()):
        raise ValueError(f"{path}: {mtllib} is not the material library of save_mesh_obj")
    return dict(vertices=np.asarray(v, np.float32).reshape(V, 3), faces=faces, vt=vt, uv_faces=uv_faces,
                uvs=vt[uv_faces] if F else np.zeros((0, 3, 2), np.float32),
                normals=np.asarray(vn, np.float32).reshape(V, 3) if vn else None, mtllib=mtllib, material=material,
                textures=textures)


def capture(active_sh_degree: int, params: Dict[str, torch.Tensor], stats, optimizer, spatial_lr_scale: float) -> Tuple:
    """GaussianModel.capture (scene/gaussian_model.py:82-123); `stats` is a densify.DensifyState (or anything with its
    five attributes)."""
    return (active_sh_degree, params["xyz"], params["f_dc"], params["f_rest"], params["scaling"], params["rotation"],
            params["opacity"], params["normal"], params["albedo"], params["roughness"], params["metallic"],
            stats.max_radii2D, stats.xyz_gradient_accum, stats.xyz_gradient_accum_abs, stats.xyz_gradient_accum_abs_max,
            stats.denom, optimizer.state_dict(), spatial_lr_scale)


def restore(model_args: Tuple):
    """GaussianModel.restore (:125-176) -> (active_sh_degree, params dict, stats dict, optimizer state_dict,
    spatial_lr_scale); the caller builds its optimizer over `params` and calls load_state_dict."""
    if len(model_args) != 18:
        raise ValueError(f"checkpoint 'gaussians' tuple has {len(model_args)} entries, expected 18")
    (deg, xyz, f_dc, f_rest, scaling, rotation, opacity, normal, albedo, roughness, metallic, max_radii2D, accum, accum_abs,
     accum_abs_max, denom, opt_dict, spatial_lr_scale) = model_args
    params = dict(xyz=xyz, f_dc=f_dc, f_rest=f_rest, opacity=opacity, normal=normal, albedo=albedo, roughness=roughness,
                  metallic=metallic, scaling=scaling, rotation=rotation)
    stats = dict(max_radii2D=max_radii2D, xyz_gradient_accum=accum, xyz_gradient_accum_abs=accum_abs,
                 xyz_gradient_accum_abs_max=accum_abs_max, denom=denom)
    return int(deg), params, stats, opt_dict, float(spatial_lr_scale)


def save_checkpoint(path: str, gaussians: Tuple, cubemap_state: Dict, light_optimizer_state: Dict, iteration: int) -> None:
    """train.py:466-490."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    torch.save({"gaussians": gaussians, "cubemap": cubemap_state, "light_optimizer": light_optimizer_state,
                "iteration": iteration}, path)


def load_checkpoint(path: str, map_location: Optional[str] = "cpu") -> Dict:
    """train.py:223-234, but with the safe loader: tensors, numbers, tuples, dicts only."""
    ckpt = torch.load(path, map_location=map_location, weights_only=True)
    for k in ("gaussians", "iteration"):
        if k not in ckpt:
            raise ValueError(f"{path}: not a GI-GS checkpoint (no '{k}')")
    return ckpt


def ply_sh_degree(path: str) -> int:
    """The SH degree a point_cloud.ply was saved with, from its f_rest_* property count (3 * ((deg + 1)^2 - 1))."""
    v = read_ply_vertices(path)
    n_rest = sum(1 for n in v if n.startswith("f_rest_"))
    K = n_rest // 3 + 1
    deg = int(round(K ** 0.5)) - 1
    if (deg + 1) ** 2 != K or n_rest % 3:
        raise ValueError(f"{path}: {n_rest} f_rest_* properties do not make a whole SH degree")
    return deg


def load_scene(path: str) -> Dict[str, np.ndarray]:
    """A trained scene from disk -- `point_cloud.ply` (GaussianModel.save_ply, scene/gaussian_model.py:397-465) or
    `chkpntN.pth` (train.py:466-490) -- as the POST-ACTIVATION arrays the rasterizer takes (the getters of
    scene/gaussian_model.py:178-263 applied on the CPU): the dictionary layout of gi-gs_amd/scenes.py
    (means3D, shs [P,K,3], opacities, normal, albedo, roughness, metallic, scales, rotations, sh_degree) + "raw"."""
    if path.endswith(".ply"):
        deg = ply_sh_degree(path)
        raw = load_ply(path, deg)
    else:
        ckpt = load_checkpoint(path)
        _, raw, _, _, _ = restore(ckpt["gaussians"])
        raw = {k: (v.detach().float().cpu() if isinstance(v, torch.Tensor) else torch.as_tensor(v)) for k, v in raw.items()}
        K = 1 + int(raw["f_rest"].shape[1])
        deg = int(round(K ** 0.5)) - 1
    F = torch.nn.functional
    f32 = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)  # noqa: E731
    return dict(means3D=f32(raw["xyz"]), shs=f32(torch.cat((raw["f_dc"], raw["f_rest"]), dim=1)),
                opacities=f32(torch.sigmoid(raw["opacity"])), normal=f32(F.normalize(raw["normal"], dim=-1)),
                albedo=f32(torch.sigmoid(raw["albedo"])), roughness=f32(torch.sigmoid(raw["roughness"])),
                metallic=f32(torch.sigmoid(raw["metallic"])), scales=f32(torch.exp(raw["scaling"])),
                rotations=f32(F.normalize(raw["rotation"])), sh_degree=deg, raw={k: f32(v) for k, v in raw.items()})
