"""CPU: the host half of the mesh export -- the PLY mesh functions of scene_io, mesh.auto_bounds -- and the numpy
restatement of the surface nets (tests/mesh_ref.py) on an analytic sphere: the restatement is what the GPU tests compare
the kernels against, so its meshes are checked here for being closed, oriented and on the sphere."""
import numpy as np
import pytest

import mesh_ref

GRIDS = [(21, 26, 23), (16, 16, 16)]


def _sphere_mesh(dims, hole=False):
    lo, h, tsdf = mesh_ref.sphere_field(dims)
    Gx, Gy, Gz = dims
    weight = np.ones_like(tsdf)
    if hole:
        weight[Gz // 2:, Gy // 2:, Gx // 2:] = 0
    rng = np.random.default_rng(3)
    attr = rng.uniform(0.0, 1.0, size=tsdf.shape + (8,)).astype(np.float32)
    return lo, h, mesh_ref.surface_nets(tsdf, weight, np.ones_like(tsdf), attr, lo, h, 1)


def test_mesh_ply_round_trip(tmp_path):
    import scene_io
    _, _, m = _sphere_mesh((16, 16, 16))
    m["albedo"][0] = (0.0, 1.0, 0.5)
    m["albedo"][1] = (-0.3, 1.7, 127.5 / 255.0)
    path = str(tmp_path / "sub" / "mesh.ply")
    scene_io.save_mesh_ply(path, **m)
    r = scene_io.read_mesh_ply(path)
    assert r["faces"].dtype == np.int32 and np.array_equal(r["faces"], m["faces"])
    for k in ("vertices", "normals", "roughness", "metallic"):
        assert r[k].dtype == np.float32 and np.array_equal(r[k], m[k]), k
    assert np.abs(r["albedo"] - np.clip(m["albedo"], 0.0, 1.0)).max() <= 1.0 / 255.0
    # the quantisation is gigs_pack_images' with bias 0.5: trunc(clamp(x * 255 + 0.5, 0, 255))
    assert (r["albedo"][0] * 255).round().tolist() == [0, 255, 128] and (r["albedo"][1] * 255).round().tolist() == [0, 255, 128]
    with open(path, "rb") as f:
        head = f.read(400).split(b"end_header")[0].decode()
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head
    assert [ln.split()[-1] for ln in head.splitlines() if ln.startswith("property") and "list" not in ln] == [
        "x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "roughness", "metallic"]
    # an empty mesh round-trips too
    e = {k: v[:0] for k, v in m.items()}
    scene_io.save_mesh_ply(path, **e)
    r = scene_io.read_mesh_ply(path)
    assert r["vertices"].shape == (0, 3) and r["faces"].shape == (0, 3)
    with pytest.raises(ValueError, match="does not exist"):
        scene_io.save_mesh_ply(path, **dict(e, faces=np.array([[0, 1, 2]])))


def test_read_ply_vertices_still_rejects_the_face_list(tmp_path):
    import scene_io
    _, _, m = _sphere_mesh((16, 16, 16))
    path = str(tmp_path / "mesh.ply")
    scene_io.save_mesh_ply(path, **m)
    with pytest.raises(ValueError, match="list properties are not supported"):
        scene_io.read_ply_vertices(path)


def test_auto_bounds_on_a_known_cloud():
    import mesh
    n = 1001
    t = np.linspace(0.0, 1.0, n)
    xyz = np.stack([t * 2.0 - 1.0, t * 4.0, t * 0.5 + 3.0], axis=1)  # uniform on [-1,1] x [0,4] x [3,3.5]
    opac = np.full((n, 1), 0.9)
    far = np.array([[100.0, 100.0, 100.0]] * 5)  # transparent outliers are ignored
    g = dict(means3D=np.concatenate([xyz, far]), opacities=np.concatenate([opac, np.full((5, 1), 0.1)]))
    lo, hi = mesh.auto_bounds(g, quantile=0.01, margin=0.05)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    span = np.array([2.0, 4.0, 0.5])
    want_lo = np.array([-1.0, 0.0, 3.0]) + 0.01 * span - 0.05 * 0.98 * span
    want_hi = np.array([1.0, 4.0, 3.5]) - 0.01 * span + 0.05 * 0.98 * span
    assert np.allclose(lo, want_lo, atol=1e-5) and np.allclose(hi, want_hi, atol=1e-5)
    lo0, hi0 = mesh.auto_bounds(g, quantile=0.0, margin=0.0)
    assert np.allclose(lo0, [-1.0, 0.0, 3.0]) and np.allclose(hi0, [1.0, 4.0, 3.5])
    with pytest.raises(ValueError, match="opacity"):
        mesh.auto_bounds(dict(means3D=far, opacities=np.full((5, 1), 0.1)))
    voxel, dims = mesh.grid_for_bounds(lo0, hi0, 41)
    assert dims == (21, 41, 6) and abs(voxel - 0.1) < 1e-9


@pytest.mark.parametrize("dims", GRIDS)
def test_restatement_meshes_the_analytic_sphere(dims):
    lo, h, m = _sphere_mesh(dims)
    figures = mesh_ref.check_closed_sphere(m["vertices"], m["faces"], h)
    print(dims, figures)
    assert np.abs(np.linalg.norm(m["normals"], axis=1) - 1.0).max() < 1e-5
    for k in ("albedo", "roughness", "metallic"):
        assert np.isfinite(m[k]).all() and m[k].min() >= 0.0 and m[k].max() <= 1.0


@pytest.mark.parametrize("dims", GRIDS)
def test_restatement_leaves_a_clean_hole_where_weights_are_zero(dims):
    _, _, m = _sphere_mesh(dims, hole=True)
    V, faces = len(m["vertices"]), m["faces"]
    assert faces.size and faces.min() >= 0 and faces.max() < V
    _, counts = mesh_ref.edge_counts(faces)
    assert counts.min() >= 1 and counts.max() <= 2
    assert (counts == 1).any()
    assert mesh_ref.euler(V, faces) == 1
