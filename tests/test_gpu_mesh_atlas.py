"""GPU: mesh texturing (csrc/mesh_atlas.hip through mesh.atlas_points / mesh.transfer_at / mesh.transfer_attributes /
mesh.bake_atlas / mesh.sample_atlas, texture_mesh.py, extract_mesh.py --texture) against its numpy restatement
(tests/mesh_atlas_ref.py).  The kernels use + - * / in float64 only, so texel points, weights and every interpolated channel
are compared as bit patterns; in the end-to-end bake the source face of a texel comes from the search, and a texel whose two
best d^2 are within 2^-40 relative in the restatement (mesh_distance_ref's `tie`) would be exempt -- the inputs leave none.
The blob's restatement searches every 4th texel (mesh_distance_ref.default_stride); test_grid_independence runs all of them
against the GPU's own one-cell grid."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_atlas_ref as ar
import mesh_clean_ref as cr
import mesh_distance_ref as dr
import mesh_simplify_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FIELDS = ("vertices", "faces", "normals", "albedo", "roughness", "metallic")


def _mesh(d):
    """A device Mesh from a mesh dict."""
    import mesh
    t = lambda k, dt: torch.from_numpy(np.ascontiguousarray(d[k], dt)).to(DEV)  # noqa: E731
    return mesh.Mesh(t("vertices", np.float32).reshape(-1, 3), t("faces", np.int32).reshape(-1, 3), t("normals", np.float32),
                     t("albedo", np.float32), t("roughness", np.float32), t("metallic", np.float32))


def _host(m):
    return {k: t.cpu().numpy() for k, t in zip(FIELDS, m)}


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _source(name):
    """(the mesh dict, the cell and origin of its simplification).  Read-only."""
    if name == "blob":
        import mesh
        lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
        vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
        vol.load(tsdf, weight, attr_weight, attr)
        d = _host(vol.extract(1))
        assert (len(d["vertices"]), len(d["faces"])) == (980, 1944)
        return d, float(np.float32(2) * np.float32(h)), None
    return sr.shared_cases()[name]


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(src dict, dst dict: mesh.simplify of src on the GPU).  Read-only."""
    import mesh
    d, cell, origin = _source(name)
    simple, report = mesh.simplify(_mesh(d), cell, origin=origin)
    assert report["faces"] > 0
    return d, _host(simple)


@functools.lru_cache(maxsize=None)
def _baked(name, B):
    """(src, dst, the restatement's bake, the GPU's bake with its report) at the default width and grid.  Read-only."""
    import mesh
    src, dst = _pair(name)
    want = ar.bake_atlas(dst, src, block=B, stride=dr.default_stride(src["faces"]))
    atlas, report = mesh.bake_atlas(_mesh(dst), _mesh(src), block=B)
    return src, dst, want, atlas, report


# ---- the points kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dr.B_CASES + ("blob",))
def test_atlas_points_equal_the_restatement(name):
    import mesh
    d = dict(_source(name)[0])
    if len(d["faces"]) % 2 == 0:
        d["faces"] = d["faces"][:-1]  # an odd F: the last block has an empty slot
    F = len(d["faces"])
    m = _mesh(d)
    for B in ar.BLOCKS:
        margin = mesh.atlas_layout(F, B).width + 1
        while margin % (B + 1) == 0:
            margin += 1
        for width in (None, margin):  # the second: margin columns right of the last whole block
            lay = mesh.atlas_layout(F, B, width)
            assert lay._asdict() == ar.atlas_layout(F, B, width) and (width is None or lay.width % (B + 1) != 0)
            want = ar.atlas_points(d["vertices"], d["faces"], lay._asdict())
            points, bary, texel_face, dest = mesh.atlas_points(m, lay)
            assert points.dtype == torch.float32 and texel_face.dtype == torch.int32 and dest.dtype == torch.int64
            assert tuple(points.shape) == (lay.n_blocks * B * (B + 1), 3) and tuple(bary.shape) == (points.shape[0], 2)
            assert np.array_equal(texel_face.cpu().numpy(), want["texel_face"]), (name, B, width)
            assert np.array_equal(dest.cpu().numpy(), want["dest"]), (name, B, width)
            assert np.array_equal(_bits(points), _bits(want["points"])), (name, B, width)
            assert np.array_equal(_bits(bary), _bits(want["bary"])), (name, B, width)
            got = dest.cpu().numpy()
            assert got.max() < lay.width * lay.height and (got == -1).sum() >= B * (B + 1) // 2
            assert np.isnan(points.cpu().numpy()[got < 0]).all() and np.isfinite(points.cpu().numpy()[got >= 0]).all()
    if name == "debris":  # the NaN vertex and the two faces with an index outside [0, V): their texels have no destination
        fc, V = np.asarray(d["faces"], np.int64), len(d["vertices"])
        bad = ~((fc >= 0) & (fc < V)).all(axis=1)
        bad[~bad] = ~np.isfinite(np.asarray(d["vertices"])[fc[~bad]]).all(axis=(1, 2))
        assert bad.sum() >= 2
        tf = texel_face.cpu().numpy()
        assert (got[np.isin(tf, np.nonzero(bad)[0])] == -1).all() and (got[(tf >= 0) & ~np.isin(tf, np.nonzero(bad)[0])] >= 0).all()


def test_an_empty_mesh_gives_an_empty_atlas_and_launches_nothing():
    import mesh
    src = _mesh(_source("cube")[0])
    empty = _mesh({k: v[:0] for k, v in _source("cube")[0].items()})
    atlas, report = mesh.bake_atlas(empty, src)
    assert atlas.layout.n_blocks == 0 and atlas.layout.height == 0 and tuple(atlas.albedo.shape) == (3, 0, atlas.layout.width)
    assert tuple(atlas.uvs.shape) == (0, 3, 2) and tuple(atlas.coverage.shape) == (0, atlas.layout.width)
    assert (report["texels"], report["baked"], report["unbaked"]) == (0, 0, 0) and json.loads(json.dumps(report)) == report
    # a source without faces: everything stays unbaked
    atlas, report = mesh.bake_atlas(src, _mesh(dict(_source("cube")[0], faces=_source("cube")[0]["faces"][:0])), block=3)
    assert report["baked"] == 0 and report["unbaked"] == report["texels"] > 0 and not bool(atlas.coverage.any())
    assert report["dims"] == [0, 0, 0] and not bool(atlas.albedo.any())
    out, face, bary, distance, report = mesh.transfer_attributes(src.vertices[:0], src, src.albedo)
    assert tuple(out.shape) == (0, 3) and report["n"] == 0


# ---- the transfer kernel alone -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _transfer_case(name):
    """(vertices, faces, points, the restatement's closest face of each).  Read-only."""
    if name == "voronoi":
        return ar.voronoi_mesh()
    d = _source(name)[0]
    v, f = d["vertices"], d["faces"]
    grid = dr.build_grid(v, f)
    points = np.concatenate(list(dr.queries(v, f, grid).values()))
    return v, f, points, dr.closest(points, v, f, grid=grid)["face"]


@pytest.mark.parametrize("name", ("voronoi", "cube", "debris", "fan", "blob"))
def test_transfer_equals_the_restatement(name):
    import mesh
    v, f, points, face = _transfer_case(name)
    V = len(v)
    z3, z1 = np.zeros((V, 3), np.float32), np.zeros(V, np.float32)
    m = _mesh(dict(vertices=v, faces=f, normals=z3, albedo=z3, roughness=z1, metallic=z1))
    p, fc = torch.from_numpy(points).to(DEV), torch.from_numpy(np.ascontiguousarray(face, np.int32)).to(DEV)
    rng = np.random.default_rng(5)
    for Cn in (1, 9, 16):
        values = rng.uniform(-3, 3, (V, Cn)).astype(np.float32)
        want = ar.transfer(points, face, v, f, values)
        out, bary, report = mesh.transfer_at(p, fc, m, torch.from_numpy(values).to(DEV))
        assert tuple(out.shape) == (len(points), Cn) and out.dtype == torch.float32
        assert report == dict(n=len(points), transferred=want["transferred"], skipped=want["skipped"])
        assert want["transferred"] > 0 and want["skipped"] == int((face < 0).sum())
        assert np.array_equal(_bits(bary), _bits(want["bary"])), (name, Cn)
        assert np.array_equal(_bits(out), _bits(want["out"])), (name, Cn)
    if name == "voronoi":  # every region of every triangle, the sliver's too
        w = want["w"]
        for k in range(len(f)):
            assert len({tuple(r) for r in (w[face == k] > 0).tolist()}) == 7, k
    else:
        assert (face < 0).sum() >= 3
        # the search and the transfer in one call: the same bits where the search found the restatement's face
        out2, face2, bary2, distance, rep = mesh.transfer_attributes(p, m, torch.from_numpy(values).to(DEV))
        same = face2.cpu().numpy() == face
        assert same.all() and rep["transferred"] == want["transferred"] and rep["skipped"] == want["skipped"]
        assert np.array_equal(_bits(out2), _bits(want["out"])) and np.array_equal(_bits(bary2), _bits(want["bary"]))
        assert rep["queries_invalid"] >= 3 and rep["far"] == 0 and json.loads(json.dumps(rep)) == rep
        assert bool((distance[face2 >= 0] >= 0).all())


def test_transfer_through_the_c_abi_touches_nothing_else():
    """gigs_mesh_transfer on the Voronoi mesh with pads of -7 around every output: a query with face -1 or dest -1 stores
    nothing, with and without destinations; a face >= F, a dest >= plane or a vertex index outside [0, V) raises the flag and
    that thread stores nothing; MeshOverflow through mesh.transfer_at."""
    import gigs_lib
    import mesh
    v, f, points, face = ar.voronoi_mesh()
    V, F, N, Cn = len(v), len(f), len(points), 9
    face = face.copy()
    face[::7] = -1
    values = np.random.default_rng(2).uniform(-1, 1, (V, Cn)).astype(np.float32)
    lib = gigs_lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    pad = 64

    def padded(n, dtype, fill=-7):
        t = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
        return t, t[pad:pad + n]

    def untouched(t, n, fill=-7):
        return bool((t[:pad] == fill).all()) and bool((t[pad + n:] == fill).all())

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    dv, df, dval, dp = up(v), up(f), up(values), up(points)
    plane = N + 11
    dest = np.arange(N, dtype=np.int64)[::-1] + 5
    dest[3::7] = -1
    for with_dest in (False, True):
        out_all, out = padded(Cn * plane if with_dest else N * Cn, torch.float32, -7.0)
        cov_all, cov = padded(plane, torch.uint8, 249)
        bary_all, bary = padded(2 * N, torch.float32, -7.0)
        counts_all, counts = padded(2, torch.int64)
        flag_all, flag = padded(1, torch.int32)
        flag.zero_()

        def run(fc, dd, faces=df):
            fc, dd = up(fc.astype(np.int32)), up(dd)  # alive until the call returns; the stream orders their reuse
            return lib.gigs_mesh_transfer(V, F, dv.data_ptr(), faces.data_ptr(), Cn, dval.data_ptr(), N, dp.data_ptr(),
                                          fc.data_ptr(), dd.data_ptr() if with_dest else None, plane,
                                          out.data_ptr(), cov.data_ptr() if with_dest else None, bary.data_ptr(),
                                          counts.data_ptr(), flag.data_ptr(), s)

        gigs_lib.check(run(face, dest), "transfer")
        want = ar.transfer(points, face, v, f, values, dest=dest if with_dest else None, plane=plane)
        assert all(untouched(t, n, fill) for t, n, fill in ((out_all, out.numel(), -7.0), (cov_all, plane, 249),
                                                          (bary_all, 2 * N, -7.0), (counts_all, 2, -7), (flag_all, 1, -7)))
        assert flag.tolist() == [0] and counts.tolist() == [want["transferred"], want["skipped"]]
        done = want["done"]
        got_bary = bary.cpu().numpy().reshape(N, 2)
        assert (got_bary[~done] == -7.0).all() and np.array_equal(_bits(got_bary[done]), _bits(want["bary"][done]))
        if with_dest:
            got, c = out.cpu().numpy().reshape(Cn, plane), cov.cpu().numpy()
            stored = np.zeros(plane, bool)
            stored[dest[done]] = True
            assert (c[stored] == 1).all() and (c[~stored] == 249).all() and (got[:, ~stored] == -7.0).all()
            assert np.array_equal(_bits(got[:, stored]), _bits(want["out"][:, stored]))
        else:
            got = out.cpu().numpy().reshape(N, Cn)
            assert (got[~done] == -7.0).all() and np.array_equal(_bits(got[done]), _bits(want["out"][done]))
            assert (cov_all == 249).all()
        # one bad row of each kind: the flag, and the bad thread stores nothing
        kinds = [("face", 1, F), ("face", 1, -2)] + ([("dest", 2, plane), ("dest", 2, -2)] if with_dest else [])
        for what, row, value in kinds:
            fc2, dd2 = face.copy(), dest.copy()
            (fc2 if what == "face" else dd2)[row] = value
            assert face[row] >= 0 and dest[row] >= 0
            out.fill_(-7.0)
            bary.fill_(-7.0)
            flag.zero_()
            gigs_lib.check(run(fc2, dd2), "transfer")
            assert flag.tolist() == [1] and untouched(out_all, out.numel(), -7.0) and untouched(bary_all, 2 * N, -7.0)
            assert (bary.cpu().numpy().reshape(N, 2)[row] == -7.0).all(), (what, value)
        broken = f.copy()
        broken[0, 1] = V
        out.fill_(-7.0)
        flag.zero_()
        gigs_lib.check(run(face, dest, up(broken)), "transfer")
        assert flag.tolist() == [1] and untouched(out_all, out.numel(), -7.0)
    z3, z1 = torch.zeros((V, 3), device=DEV), torch.zeros(V, device=DEV)
    m = mesh.Mesh(dv, df, z3, z3.clone(), z1, z1.clone())
    bad = up(np.where(np.arange(N) == 4, F, face).astype(np.int32))
    with pytest.raises(mesh.MeshOverflow):
        mesh.transfer_at(dp, bad, m, dval)
    with pytest.raises(ValueError, match="values"):
        mesh.transfer_at(dp, up(face.astype(np.int32)), m, torch.zeros((V, 17), device=DEV))


# ---- end to end --------------------------------------------------------------------------------------------------------------
CASES = [("cube", 3), ("cube", 8), ("fan", 4), ("fan", 8), ("blob", 4)]


@pytest.mark.parametrize("name,B", CASES)
def test_bake_atlas_equals_the_restatement(name, B):
    src, dst, want, atlas, report = _baked(name, B)
    assert int(want["closest"]["tie"].sum()) == 0, "the inputs are chosen to leave no tie open"
    lay = atlas.layout
    assert lay._asdict() == want["layout"] and json.loads(json.dumps(report)) == report
    W, H = lay.width, lay.height
    for k, t in (("albedo", atlas.albedo), ("orm", atlas.orm), ("normal", atlas.normal)):
        assert tuple(t.shape) == (3, H, W) and t.dtype == torch.float32, k
    assert tuple(atlas.coverage.shape) == (H, W) and atlas.coverage.dtype == torch.uint8
    assert np.array_equal(atlas.uvs.cpu().numpy(), ar.face_uvs(len(dst["faces"]), want["layout"]))
    got = torch.cat((atlas.albedo, atlas.orm, atlas.normal), 0).cpu().numpy().reshape(9, H * W)
    cov = atlas.coverage.cpu().numpy().reshape(-1)
    # the texels the restatement searched, and every texel that belongs to no face
    searched = np.zeros(H * W, bool)
    searched[want["dest"][want["searched"] & (want["dest"] >= 0)]] = True
    none = np.ones(H * W, bool)
    none[want["dest"][want["dest"] >= 0]] = False
    check = searched | none
    assert (cov[none] == 0).all() and (got[:, none] == 0).all() and check.sum() > 0.2 * H * W
    assert np.array_equal(cov[check], want["coverage"].reshape(-1)[check])
    assert np.array_equal(_bits(got[:, check]), _bits(want["planes"].reshape(9, -1)[:, check])), (name, B)
    assert (got[3][cov == 1] == 1.0).all(), "occlusion=None bakes 1"
    assert report["baked"] + report["unbaked"] == W * H == report["texels"] and report["baked"] == int(cov.sum())
    assert report["far"] == 0 and report["faces_skipped"] == 0 and report["block"] == B and report["width"] == W
    assert report["queries_invalid"] == int((want["dest"] < 0).sum()) and report["baked"] == int((want["dest"] >= 0).sum())
    if dr.default_stride(src["faces"]) == 1:
        assert report["baked"] == want["transferred"]
        d = want["closest"]["d"][want["closest"]["face"] >= 0]
        assert abs(report["distance_mean"] - d.mean()) <= 2.0 ** -20 * max(d.max(), 1e-30) and abs(report["distance_max"] - d.max()) <= 2.0 ** -22 * max(d.max(), report["cell"])
    print("%s B=%d: %d x %d, %d baked of %d texels, %d compared; texel to source mean %.3e max %.3e"
          % (name, B, W, H, report["baked"], W * H, int(check.sum()), report["distance_mean"], report["distance_max"]))


@pytest.mark.parametrize("name", ("cube", "fan", "blob"))
def test_grid_independence_and_determinism(name):
    """Three cell sizes and a repeated call give the bits of the one-cell grid, the GPU's own brute force, on every texel."""
    import mesh
    src, dst, _, atlas, report = _baked(name, 4)
    s, d = _mesh(src), _mesh(dst)
    one, r1 = mesh.bake_atlas(d, s, block=4, cell=1e6 * report["cell"])
    assert r1["dims"] == [1, 1, 1]
    planes1 = torch.cat((one.albedo, one.orm, one.normal), 0)
    for scale in (0.5, 1.0, 3.0):
        for _ in range(2):
            a, r = mesh.bake_atlas(d, s, block=4, cell=scale * report["cell"])
            assert torch.equal(torch.cat((a.albedo, a.orm, a.normal), 0).view(torch.int32), planes1.view(torch.int32)), (name, scale)
            assert torch.equal(a.coverage, one.coverage) and r["baked"] == r1["baked"]
    grid = mesh.triangle_grid(s)
    a, r = mesh.bake_atlas(d, s, block=4, grid=grid)
    assert torch.equal(a.albedo.view(torch.int32), atlas.albedo.view(torch.int32)) and r == report
    assert torch.equal(a.albedo.view(torch.int32), one.albedo.view(torch.int32))


def test_max_distance_leaves_far_texels_unbaked():
    import mesh
    src, dst, want, atlas, report = _baked("fan", 4)
    d = want["closest"]["d"]
    limit = float(np.median(d[np.isfinite(d)]))
    assert limit > 0
    capped = ar.bake_atlas(dst, src, block=4, max_distance=limit)
    a, r = mesh.bake_atlas(_mesh(dst), _mesh(src), block=4, max_distance=limit)
    assert int(capped["closest"]["tie"].sum()) == 0
    assert r["far"] == capped["closest"]["far"] > 0 and r["baked"] == capped["transferred"] < report["baked"]
    assert np.array_equal(a.coverage.cpu().numpy(), capped["coverage"])
    assert np.array_equal(_bits(torch.cat((a.albedo, a.orm, a.normal), 0)), _bits(capped["planes"]))
    assert r["distance_max"] <= limit * (1.0 + 2.0 ** -22)
    with pytest.raises(ValueError, match="max_distance"):
        mesh.bake_atlas(_mesh(dst), _mesh(src), max_distance=-1.0)


def test_occlusion_channel():
    """occlusion=None: the O plane is 1 where baked, 0 elsewhere.  A tensor: interpolated like the other channels."""
    import mesh
    src, dst, want, atlas, _ = _baked("cube", 8)
    cov = atlas.coverage.bool()
    assert bool((atlas.orm[0][cov] == 1.0).all()) and bool((atlas.orm[0][~cov] == 0.0).all())
    occ = np.random.default_rng(9).uniform(0, 1, len(src["vertices"])).astype(np.float32)
    wanted = ar.bake_atlas(dst, src, block=8, occlusion=occ)
    a, r = mesh.bake_atlas(_mesh(dst), _mesh(src), block=8, occlusion=torch.from_numpy(occ).to(DEV))
    assert np.array_equal(_bits(a.orm), _bits(wanted["planes"][3:6])) and torch.equal(a.coverage, atlas.coverage)
    assert torch.equal(a.albedo, atlas.albedo) and torch.equal(a.normal, atlas.normal) and torch.equal(a.orm[1:], atlas.orm[1:])
    o = a.orm[0][cov]
    assert float(o.min()) >= 0.0 and float(o.max()) <= 1.0 and float(o.std()) > 0.05
    with pytest.raises(ValueError, match="occlusion"):
        mesh.bake_atlas(_mesh(dst), _mesh(src), occlusion=torch.from_numpy(occ[:-1]).to(DEV))


def test_linear_attributes_come_back_exactly():
    """Independent of the restatement: the jittered plane baked onto itself with attributes that are linear in the position,
    a . x + b with a, b > 0 on x in [0, 1]^3 (the jitter reaches a little below 0).  A linear function survives the
    interpolation on the source face, the (extrapolated) texel points and the bilinear lookup, so sample_atlas at 4 097
    surface samples of the faces with no vertex on the border (a gutter texel of such a face lies on a neighbour in the
    plane) equals a . x + b at the sample but for float32: the texel point and the sample point are float32 roundings of
    positions (2^-24 M each, M = the largest value), the texels are stored as float32 (2^-24 M), the sample's float32
    barycentrics move its UV by 2^-24 of a chart (6 texels here, a gradient of at most M / 6 per texel: 2^-24 M), and the
    float32 v of the UV (u is exact: W is a power of two) moves the lookup by at most H 2^-25 texels, 2^-25 H M / 6 in
    value as long as the taps stay the face's own -- which every sample at least 2^-18 texel inside its chart's rows
    does, and the test asserts that of its samples.  The source's own table is a float32 rounding of a . x + b (2^-24 M).
    With H = 40 that is (5 + 40 / 12) 2^-24 M = 0.52 2^-20 M: inside the 2^-20 M asked for.  Measured on an MI355X: 2.24e-07, 0.090 of the tolerance."""
    import mesh
    d = dict(sr.shared_cases()["plane"][0])
    v, f = d["vertices"].astype(np.float64), np.asarray(d["faces"], np.int64)
    rng = np.random.default_rng(4)
    A, b = rng.uniform(0.25, 1.0, (9, 3)), rng.uniform(0.5, 1.0, 9)
    lin = (v @ A.T + b).astype(np.float32)  # the per-vertex table the source carries, rounded once
    d.update(albedo=lin[:, 0:3], roughness=lin[:, 4], metallic=lin[:, 5], normals=lin[:, 6:9])
    m = _mesh(d)
    atlas, report = mesh.bake_atlas(m, m, block=8, occlusion=torch.from_numpy(lin[:, 3].copy()).to(DEV))
    assert (atlas.layout.width, atlas.layout.height) == (128, 40) and report["baked"] == len(f) * 36
    n = int(round(len(v) ** 0.5))
    i, j = np.arange(len(v)) // n, np.arange(len(v)) % n
    inner = (i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)
    keep = np.nonzero(inner[f].all(axis=1))[0]
    assert len(keep) == 2 * (n - 3) ** 2 > 0
    sub = _mesh(dict(d, faces=d["faces"][keep]))
    points, face, bary = mesh.sample_surface(sub, 4097, 3)
    face = torch.from_numpy(keep).to(DEV)[face.long()]
    w = torch.cat((1.0 - bary.double().sum(1, keepdim=True), bary.double()), 1)
    assert float(w.min()) * 6 > 2.0 ** -18, "a sample within 2^-18 texel of its chart's border"
    planes = torch.cat((atlas.albedo, atlas.orm, atlas.normal), 0)
    got = mesh.sample_atlas(planes, atlas.layout, face, bary).cpu().numpy()
    want = points.cpu().numpy().astype(np.float64) @ A.T + b
    M = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print("plane onto itself: %d samples on %d inner faces, largest difference %.3e = %.3f of 2^-20 max|value| (%.3e)"
          % (len(got), len(keep), err, err / (2.0 ** -20 * M), 2.0 ** -20 * M))
    assert got.shape == (4097, 9) and err <= 2.0 ** -20 * M
    # the lookup is the restatement's
    ref = ar.sample_atlas(planes.cpu().numpy(), atlas.layout._asdict(), face.cpu().numpy(), bary.cpu().numpy())
    assert np.abs(got - ref).max() <= 2.0 ** -45 * M


# ---- the tools ---------------------------------------------------------------------------------------------------------------
def _png_size(path):
    import struct
    head = open(path, "rb").read(26)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    return struct.unpack(">II", head[16:24])


def test_texture_mesh_tool(tmp_path):
    import mesh
    import scene_io
    import texture_mesh
    src, _ = _pair("blob")
    raw = str(tmp_path / "raw.ply")
    scene_io.save_mesh_ply(raw, *(src[k] for k in FIELDS))
    out = str(tmp_path / "light" / "blob.obj")
    rep = texture_mesh.texture_mesh([raw, "-o", out, "--cell_edges", "2", "--block", "4", "--samples", "4097"])
    assert json.loads(json.dumps(rep)) == rep and rep["path"] == out and rep["occlusion"] == "none"
    at = rep["atlas"]
    W, H = at["width"], at["height"]
    assert at["baked"] + at["unbaked"] == W * H and at["baked"] == rep["faces"] * 10 and at["block"] == 4
    lay = mesh.atlas_layout(rep["faces"], 4)
    assert (W, H) == (lay.width, lay.height) and rep["simplify"]["faces"] == rep["faces"] and rep["faces"] < len(src["faces"])
    folder = os.path.dirname(out)
    for k in ("albedo", "orm", "roughness", "metallic", "normal"):
        path = os.path.join(folder, "blob_%s.png" % k)
        assert rep["files"][k] == path and _png_size(path) == (W, H), k
    assert os.path.exists(os.path.join(folder, "blob.mtl"))
    obj = scene_io.read_mesh_obj(out)
    assert len(obj["faces"]) == rep["faces"] and len(obj["vertices"]) == rep["vertices"] and len(obj["vt"]) == 3 * rep["faces"]
    assert np.array_equal(obj["uvs"], mesh.face_uvs(rep["faces"], lay).numpy()) and obj["normals"] is not None
    assert obj["textures"]["albedo"] == "blob_albedo.png" and obj["textures"]["normal"] == "blob_normal.png"
    s = rep["samples"]
    assert s["n"] == 4097 and s["compared"] == 4097
    for name, _, _ in texture_mesh.GROUPS:
        assert s[name]["atlas_rms"] >= 0 and s[name]["vertex_rms"] >= 0, name
    assert s["occlusion"]["atlas_rms"] <= 1e-12 and s["occlusion"]["vertex_rms"] <= 1e-12  # 1 everywhere, up to the weights' sum
    print("blob at 2 edges, B = 4: " + ", ".join("%s atlas %.4f vertex %.4f" % (k, s[k]["atlas_rms"], s[k]["vertex_rms"])
                                                 for k, _, _ in texture_mesh.GROUPS))
    # a light mesh from a file, the source's occlusion channel, a margin width; the texels are mesh.bake_atlas's
    baked = str(tmp_path / "baked.ply")
    occ = np.random.default_rng(1).uniform(0, 1, len(src["vertices"])).astype(np.float32)
    scene_io.save_mesh_ply(baked, *(src[k] for k in FIELDS), occlusion=occ)
    import simplify_mesh
    low = simplify_mesh.simplify_mesh([raw, "-o", str(tmp_path / "low.ply"), "--cell_edges", "2"])
    out2 = str(tmp_path / "second.obj")
    rep2 = texture_mesh.texture_mesh([baked, "-o", out2, "--target", low["path"], "--block", "3", "--width", "250"])
    assert rep2["occlusion"] == "channel" and "simplify" not in rep2 and "samples" not in rep2 and rep2["faces"] == rep["faces"]
    assert _png_size(str(tmp_path / "second_orm.png")) == (250, rep2["atlas"]["height"])
    with pytest.raises(ValueError, match=".obj"):
        texture_mesh.texture_mesh([raw, "-o", str(tmp_path / "x.ply"), "--cell_edges", "2"])


def test_extract_mesh_texture(tmp_path):
    """extract_mesh.py --texture on the blob scene of test_gpu_mesh_raycast.py's set-up: the default output is the same bytes
    with and without the option, and --simplify 2 --texture 4 -o x.obj writes the simplified mesh textured from the raw
    level set."""
    from argparse import Namespace

    import densify
    import extract_mesh
    import mesh
    import optim
    import relight
    import scene_io
    import scenes
    import synthetic_dataset
    import train_iteration as ti
    src = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=6, size=64)
    out = str(tmp_path / "run")
    os.makedirs(out)
    raw = ti.raw_from_scene(scenes.surface_scene(P=4000, sh_degree=0, seed=3, scale_mu=0.05), DEV)
    opt = optim.FusedAdam([{"params": [raw[k]], "lr": 0.0, "name": k} for k in raw], lr=0.0, eps=1e-15)
    light = relight.make_light(torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(DEV) * 0.5, res=256)
    ck = os.path.join(out, "chkpnt7.pth")
    scene_io.save_checkpoint(ck, scene_io.capture(0, raw, densify.DensifyState(raw["xyz"].shape[0], DEV), opt, 1.0),
                             light.state_dict(), {}, 7)
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=src, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    assert extract_mesh.parse_args(["-m", out, "--checkpoint", ck]).texture == 0
    base = ["-m", out, "--checkpoint", ck, "--grid", "40", "--split", "test", "--simplify", "2", "--bake_occlusion", "64"]
    r0 = extract_mesh.extract_mesh(base + ["-o", "plain.ply"])
    r1 = extract_mesh.extract_mesh(base + ["--texture", "0", "-o", "plain0.ply"])
    assert sorted(r0) == sorted(r1) and "texture" not in r0
    assert open(r0["path"], "rb").read() == open(r1["path"], "rb").read()
    r2 = extract_mesh.extract_mesh(base + ["--texture", "4", "-o", "light.obj"])
    assert json.loads(json.dumps(r2)) == r2 and (r2["vertices"], r2["faces"]) == (r0["vertices"], r0["faces"])
    t = r2["texture"]
    assert t["block"] == 4 and t["baked"] + t["unbaked"] == t["width"] * t["height"] and t["baked"] == 10 * r2["faces"]
    assert r2["occlusion"]["n"] > r0["occlusion"]["n"], "the occlusion is baked on the level set, not on the simplified mesh"
    obj = scene_io.read_mesh_obj(r2["path"])
    plain = scene_io.read_mesh_ply(r0["path"])
    assert np.array_equal(obj["faces"], plain["faces"]) and np.array_equal(_bits(obj["vertices"]), _bits(plain["vertices"]))
    assert np.array_equal(obj["uvs"], mesh.face_uvs(r2["faces"], mesh.atlas_layout(r2["faces"], 4)).numpy())
    for k in ("albedo", "orm", "roughness", "metallic", "normal"):
        assert _png_size(r2["files"][k]) == (t["width"], t["height"]), k
    for bad in (["--texture", "4", "-o", "x.ply"], ["--texture", "2", "-o", "x.obj"]):
        with pytest.raises(ValueError, match="--texture"):
            extract_mesh.extract_mesh(base + bad)
    with pytest.raises(ValueError, match="--texture"):
        extract_mesh.extract_mesh(["-m", out, "--checkpoint", ck, "--grid", "40", "--split", "test", "--texture", "4", "-o", "x.obj"])
