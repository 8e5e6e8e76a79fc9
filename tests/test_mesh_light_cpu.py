"""CPU: the numpy restatement of light baking (tests/mesh_light_ref.py) against its own brute force and against the analytic
irradiance of a linear sky, the argument checks of mesh.trace_hemispheres / mesh.gather_light / mesh.sky_cube that need no
GPU, and the PLY's irradiance channels."""
import numpy as np
import pytest
import torch

import mesh_light_ref as lr
import mesh_raycast_ref as rr


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cases():
    v, f, n, _ = rr.crease()
    return dict(open_box=lr.open_box() + ({},), crease=(v, f, n, dict(bias=1e-3, seed=9)))


@pytest.mark.parametrize("name", ["open_box", "crease"])
def test_trace_equals_brute_force(name):
    """The restated trace through the grid at four cell sizes (the last: one cell) equals every usable face tested for every
    ray: records and weights, bit for bit."""
    v, f, n, kw = _cases()[name]
    table = rr.direction_table(64, 4)
    kw = dict(kw, bias=kw.get("bias", lr.default_bias(rr.build_grid(v, f))))
    want = lr.trace(v, f, n, table, brute=True, **kw)
    assert want["front_hits"] > 0 and want["misses"] > 0
    for cell in rr.cell_sizes(v, f):
        got = lr.trace(v, f, n, table, cell=cell, **kw)
        assert np.array_equal(got["face"], want["face"]) and np.array_equal(_bits(got["bary"]), _bits(want["bary"])), cell
        assert all(got[k] == want[k] for k in ("misses", "front_hits", "back_hits", "no_normal"))
    assert want["misses"] + want["front_hits"] + want["back_hits"] == 64 * len(v)


def test_records_and_passes_of_the_open_box():
    v, f, n = lr.open_box()
    table = rr.direction_table(64, 4)
    tr = lr.trace(v, f, n, table)
    assert tr["back_hits"] == 0 and tr["no_normal"] == 0  # the faces front the interior
    closed = lr.trace(*rr.box_interior(), table)
    assert closed["back_hits"] == 64 * len(v) and (closed["face"] <= -2).all()  # outward faces seen from inside
    c = np.array([0.7, 1.3, 5e3], np.float32)
    sky = np.ascontiguousarray(np.broadcast_to(c, (6, 4, 4, 3)))
    I, Q = lr.light(v, f, n, table, 0, tr["face"], tr["bary"], sky, np.ones((len(v), 3), np.float32), bounces=4)
    assert (I[1:] >= I[:-1]).all() and (I.astype(np.float64) <= c.astype(np.float64) * (1.0 + 2.0 ** -20)).all()
    assert np.array_equal(_bits(Q), _bits(I))  # reflectance 1
    share = (tr["face"] == -1).sum(axis=1) / 64.0
    assert np.array_equal(_bits(I[0]), _bits((share[:, None] * c.astype(np.float64)).astype(np.float32)))
    I0, _ = lr.light(v, f, n, table, 0, closed["face"], closed["bary"], sky, np.ones((len(v), 3), np.float32), bounces=2)
    assert (I0 == 0).all()


def test_sky_texel_convention():
    """Faces +x -x +y -y +z -z, and on each the (u, v) signs of cube_face_uv."""
    d = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0.9, -0.9], [0.9, 1, 0.9]], np.float64)
    face, iy, ix = lr.sky_texel(d, 4)
    assert face.tolist() == [0, 1, 2, 3, 4, 5, 0, 2]
    assert (ix[:6] == 2).all() and (iy[:6] == 2).all()  # the centre: u = v = 1/2, floor(2.0)
    assert (int(ix[6]), int(iy[6])) == (3, 0)  # +x: u = -z / 2|x| + 1/2, v = -y / 2|x| + 1/2
    assert (int(ix[7]), int(iy[7])) == (3, 3)  # +y: u = x / 2|y| + 1/2, v = z / 2|y| + 1/2
    assert [int(a[0]) for a in lr.sky_texel(np.zeros((1, 3)), 4)] == [0, 0, 0]  # d = 0: a NaN goes to texel 0
    lr.texel_centres(8)  # asserts the round trip of every texel


def test_analytic_irradiance_of_the_restatement():
    nrm = lr.analytic_normals()
    V = len(nrm)
    sky = lr.linear_sky(lr.ANALYTIC_A, lr.ANALYTIC_B, 256)
    table = rr.direction_table(1024, 16)
    assert np.array_equal(table[:, :, 2] >= 0, np.ones((16, 1024), bool))
    want, bound = lr.analytic_irradiance(nrm)
    for seed in (0, 1):
        I, _ = lr.gather(np.zeros((V, 3), np.float32), np.zeros((0, 3), np.int32), nrm, table, seed, np.full((V, 1024), -1, np.int32),
                         np.zeros((V, 1024, 2), np.float32), sky, np.zeros((V, 3), np.float32))
        err = np.abs(I.astype(np.float64) - want)
        print("seed %d: largest error per channel %s, bound %s" % (seed, err.max(axis=0), bound))
        assert (err <= bound).all()
    # the first term of the bound: the first moment of every rotation of the table
    mean = table.astype(np.float64).mean(axis=1)
    assert np.abs(mean[:, :2]).max() <= 5.2e-4 and np.abs(mean[:, 2] - 2.0 / 3.0).max() <= 1.9e-6


def test_arguments():
    import mesh
    v, f, n = lr.open_box()
    z1 = torch.zeros(len(v))
    m = mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), torch.zeros((len(v), 3)), z1, z1.clone())
    for bad in (dict(rays=65), dict(rays=32), dict(rays=2048), dict(rotations=0), dict(rotations=65), dict(max_distance=-1.0),
                dict(bias=float("nan")), dict(directions=np.zeros((4, 64, 2), np.float32))):
        with pytest.raises(ValueError, match="trace_hemispheres"):
            mesh.trace_hemispheres(m, **bad)
    with pytest.raises(ValueError, match="memory_limit"):
        mesh.trace_hemispheres(m, rays=64, memory_limit=12 * 64 * len(v) - 1)
    with pytest.raises(RuntimeError, match="no CPU path"):  # everything else in order: the device is what is wrong
        mesh.trace_hemispheres(m, rays=64, memory_limit=12 * 64 * len(v))
    with pytest.raises(RuntimeError, match="no CPU path"):  # a malformed mesh gets the mesh check's message, not an AttributeError
        mesh.trace_hemispheres(m._replace(vertices=None), rays=64)
    with pytest.raises(RuntimeError, match="vertices must be"):
        mesh.trace_hemispheres(m._replace(vertices=torch.zeros(5)), rays=64)
    hits = mesh.HemisphereHits(torch.full((len(v), 64), -1, dtype=torch.int32), torch.zeros((len(v), 64, 2)),
                               mesh.occlusion_directions(64, 4), 0, 64, 4)
    good = torch.ones((6, 4, 4, 3))
    with pytest.raises(ValueError, match="bounces"):
        mesh.gather_light(m, hits, good, bounces=-1)
    for cube in (good.numpy(), torch.ones((6, 4, 4)), torch.ones((6, 4, 5, 3)), torch.ones((5, 4, 4, 3)), good.double(),
                 torch.ones((6, 4, 4, 4))):
        with pytest.raises(ValueError, match="cube"):
            mesh.gather_light(m, hits, cube)
    for value in (float("nan"), float("inf"), -1e-3):
        cube = good.clone()
        cube[3, 1, 2, 0] = value
        with pytest.raises(ValueError, match="finite and >= 0"):
            mesh.gather_light(m, hits, cube)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.gather_light(m, hits, good)
    assert mesh.TRACE_MEMORY_LIMIT == 8 << 30


def test_sky_cube():
    import mesh
    base = torch.arange(6 * 8 * 8 * 3, dtype=torch.float32).reshape(6, 8, 8, 3) - 40.0
    sky = mesh.sky_cube(base, 4)
    assert tuple(sky.shape) == (6, 4, 4, 3) and float(sky.min()) == 0.0
    want = base.reshape(6, 4, 2, 4, 2, 3).mean(dim=(2, 4)).clamp_min(0.0)
    assert torch.equal(sky, want)
    assert torch.equal(mesh.sky_cube(base, 8), base.clamp_min(0.0)) and torch.equal(mesh.sky_cube(base, 32), base.clamp_min(0.0))

    class Light:
        pass
    light = Light()
    light.base = torch.nn.Parameter(base.clone())
    assert torch.equal(mesh.sky_cube(light, 4), want) and not mesh.sky_cube(light, 4).requires_grad
    for bad in (dict(res=3), dict(res=0)):
        with pytest.raises(ValueError):
            mesh.sky_cube(base, **bad)
    with pytest.raises(ValueError):
        mesh.sky_cube(torch.zeros((6, 8, 4, 3)))


def test_ply_round_trip(tmp_path):
    import scene_io
    rng = np.random.default_rng(0)
    V = 7
    v, n, a = (rng.uniform(size=(V, 3)).astype(np.float32) for _ in range(3))
    r, m, occ = (rng.uniform(size=V).astype(np.float32) for _ in range(3))
    f = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]], np.int32)
    irr = (rng.uniform(size=(V, 3)) * 1e4).astype(np.float32)
    irr[0] = [0.0, 1e-30, 3e38]
    paths = {k: str(tmp_path / (k + ".ply")) for k in ("plain", "none", "occ", "occ_none", "both", "irr")}
    scene_io.save_mesh_ply(paths["plain"], v, f, n, a, r, m)
    scene_io.save_mesh_ply(paths["none"], v, f, n, a, r, m, irradiance=None)
    scene_io.save_mesh_ply(paths["occ"], v, f, n, a, r, m, occ)
    scene_io.save_mesh_ply(paths["occ_none"], v, f, n, a, r, m, occlusion=occ, irradiance=None)
    scene_io.save_mesh_ply(paths["both"], v, f, n, a, r, m, occlusion=occ, irradiance=irr)
    scene_io.save_mesh_ply(paths["irr"], v, f, n, a, r, m, irradiance=torch.from_numpy(irr))
    raw = {k: open(p, "rb").read() for k, p in paths.items()}
    assert raw["plain"] == raw["none"] and raw["occ"] == raw["occ_none"] and b"irradiance" not in raw["occ"]
    assert len(raw["both"]) - len(raw["occ"]) == 12 * V + len(b"property float irradiance_r\n") * 3
    both, only, plain = (scene_io.read_mesh_ply(paths[k]) for k in ("both", "irr", "plain"))
    assert np.array_equal(_bits(both["irradiance"]), _bits(irr)) and np.array_equal(_bits(both["occlusion"]), _bits(occ))
    assert np.array_equal(_bits(only["irradiance"]), _bits(irr)) and "occlusion" not in only and "irradiance" not in plain
    header = raw["both"].split(b"end_header")[0].decode().split("\n")
    assert header[header.index("property float occlusion") + 1:][:3] == ["property float irradiance_" + c for c in "rgb"]
    for k in ("vertices", "faces", "normals", "albedo", "roughness", "metallic"):
        assert np.array_equal(both[k], plain[k]) and np.array_equal(only[k], plain[k])
    with pytest.raises(ValueError, match="irradiance"):
        scene_io.save_mesh_ply(paths["irr"], v, f, n, a, r, m, irradiance=irr[:, :2])


def test_render_mesh_lighting_arguments():
    import render_mesh
    a = render_mesh.parse_args(["-m", "o", "--mesh", "m.ply", "--hdri", "a.hdr"])
    assert (a.lighting, a.bounces, a.sky_res, a.light_rays) == ("screen", 1, 32, 256) and render_mesh._check(a) == 0
    a = render_mesh.parse_args(["-m", "o", "--mesh", "m.ply", "--hdri", "a.hdr", "--lighting", "baked", "--bounces", "3"])
    assert (a.lighting, a.bounces) == ("baked", 3) and render_mesh._check(a) == 0
    for argv in (["-m", "o", "--mesh", "m.ply", "--checkpoint", "c.pth", "--lighting", "baked"],
                 ["-m", "o", "--mesh", "m.obj", "--hdri", "a.hdr", "--lighting", "baked"],
                 ["-m", "o", "--mesh", "m.ply", "--hdri", "a.hdr", "--lighting", "baked", "--bounces", "-1"]):
        with pytest.raises(ValueError, match="lighting baked|bounces"):
            render_mesh._check(render_mesh.parse_args(argv))
    with pytest.raises(SystemExit):
        render_mesh.parse_args(["-m", "o", "--mesh", "m.ply", "--hdri", "a.hdr", "--lighting", "both"])
