"""Triangle meshes of the TSDF volume on the GPU (include/cspm.h "TSDF meshes") held to tests/tsdfmesh_ref.py bit
for bit: vertices, faces and both counts of fields put on the device by cspm_tsdf_set_volume -- one cell in several cases, volumes
without cells, cells whose i+1 column belongs to the next wave and the next workgroup, noise with unknown voxels and with 0.0, -0.0 and
NaN, a sphere over 2304 workgroups -- and of integrated views against the one-shot entry; capacities, the host and device variants, the
volume round trip, a second call, the memory of the first call, the timing bracket, the errors, the command line and an unchanged
PatchMatch run."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_ref as tr
import tsdfmesh_ref as mr
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3
ORIGIN, VOXEL = (-1.0, 0.5, 2.0), 0.25


@pytest.fixture(autouse=True, scope="module")
def _torch_first(_gpu_ctx_session):
    """PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py)"""
    yield


def _one_cell(case):
    return np.array([1.0 if (case >> c) & 1 else -1.0 for c in range(8)], np.float32).reshape(2, 2, 2), None


def _noise(dims, seed, unknown=0.0, special=False):
    D = mr.noise_volume(seed, dims)
    rng = np.random.default_rng(100 + seed)
    W = None
    if special:
        u = rng.uniform(size=D.shape)
        D[u < 0.03] = 0.0
        D[(u >= 0.03) & (u < 0.06)] = -0.0
        D[(u >= 0.06) & (u < 0.09)] = np.nan
    if unknown:
        W = np.where(rng.uniform(size=D.shape) < unknown, 0.0, rng.integers(1, 5, size=D.shape)).astype(np.float32)
    return D, W


def _sphere():
    """a sphere of radius 20 voxels in 96 x 96 x 64: 2304 workgroups, the scan's three passes with a carry"""
    z, y, x = np.mgrid[0:64, 0:96, 0:96].astype(np.float64)
    return (np.sqrt((x - 47.3) ** 2 + (y - 46.1) ** 2 + (z - 30.7) ** 2) - 20.0).astype(np.float32), None


FIELDS = {f"2x2x2_case_{c:#04x}": functools.partial(_one_cell, c) for c in (0, 255, 0x69, 1, 254, 0x5b, 0x96, 0x3c, 0x7e)}
FIELDS.update({
    "1x4x4": functools.partial(_noise, (1, 4, 4), 1),
    "4x4x1": functools.partial(_noise, (4, 4, 1), 2),
    "3x2x2": functools.partial(_noise, (3, 2, 2), 3),
    "65x3x2": functools.partial(_noise, (65, 3, 2), 4),        # the cell at i = 63: its i+1 corners and vertices belong to the next wave
    "257x2x2": functools.partial(_noise, (257, 2, 2), 5),      # the cell at i = 255: the next workgroup
    "33x17x9_noise": functools.partial(_noise, (33, 17, 9), 7),
    "33x17x9_noise_unknown": functools.partial(_noise, (33, 17, 9), 7, 0.05),
    "33x17x9_noise_special": functools.partial(_noise, (33, 17, 9), 7, 0.03, True),
    "96x96x64_sphere": _sphere,
})


@functools.lru_cache(maxsize=None)
def _field(name):
    """-> D, W, C, the restatement's mesh (computed once and shared; nobody writes into it)"""
    D, W = FIELDS[name]()
    if W is None:
        W = np.ones(D.shape, np.float32)
    rng = np.random.default_rng(len(name))
    Cc = rng.integers(0, 256, size=D.shape + (4,)).astype(np.uint8)
    Cc[..., 3] = rng.uniform(size=D.shape) < 0.8
    return D, W, Cc, mr.mesh(mr.volume(D, W, Cc, ORIGIN, VOXEL))


def _same_mesh(got, want, what, vcap=None, fcap=None):
    assert got["n_vertices"] == want["n_vertices"], f"{what}: {got['n_vertices']} vertices, {want['n_vertices']} expected"
    assert got["n_faces"] == want["n_faces"], f"{what}: {got['n_faces']} faces, {want['n_faces']} expected"
    if "vertices" in got:
        ref = want["vertices"] if vcap is None else want["vertices"][:vcap]
        assert len(got["vertices"]) == len(ref), f"{what}: {len(got['vertices'])} vertex records, {len(ref)} expected"
        for name in tr.POINT.names:
            assert tr.same_bits(got["vertices"][name], ref[name]), f"{what}: vertex field {name} differs in {np.sum(got['vertices'][name] != ref[name])} records"
    if "faces" in got:
        ref = want["faces"] if fcap is None else want["faces"][:fcap]
        assert len(got["faces"]) == len(ref), f"{what}: {len(got['faces'])} face records, {len(ref)} expected"
        assert np.array_equal(got["faces"]["v"], ref["v"]), f"{what}: {np.sum(np.any(got['faces']['v'] != ref['v'], 1))} faces differ"


class _Volume:
    """a volume of the given field on the device, ended on exit"""

    def __init__(self, ctx, D, W=None, Cc=None):
        self.ctx = ctx
        nz, ny, nx = D.shape
        ctx.tsdf_begin(ORIGIN, VOXEL, (nx, ny, nz))
        try:
            ctx.tsdf_set_volume(D, np.ones(D.shape, np.float32) if W is None else W, Cc)
        except Exception:
            ctx.tsdf_end()
            raise

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.tsdf_end()


@pytest.mark.parametrize("name", list(FIELDS))
def test_set_volume_mesh_against_the_restatement(gpu_ctx, name):
    D, W, Cc, want = _field(name)
    if name.startswith("2x2x2"):
        assert want["n_faces"] == len(mr.table()[int(name[-4:], 16)])
    elif name in ("1x4x4", "4x4x1"):
        assert want["n_faces"] == 0 and want["n_vertices"] > 0
    elif name == "33x17x9_noise":
        assert len(set(want["cases"].tolist())) == 256
    elif name == "33x17x9_noise_special":
        assert want["unknown_cells"] > 50 and np.isnan(D).sum() > 50 and (D == 0.0).sum() > 100
    elif name == "96x96x64_sphere":
        assert want["n_faces"] > 5000 and mr.euler(want["all_faces"]) == 2
    else:
        assert want["n_faces"] > 0
    with _Volume(gpu_ctx, D, W, Cc) as ctx:
        _same_mesh(ctx.tsdf_mesh(), want, name)
        # the vertices are the surface points, record for record
        pts = ctx.tsdf_points()
        assert pts["count"] == want["n_vertices"]
        for field in tr.POINT.names:
            assert tr.same_bits(pts["cloud"][field], want["vertices"][field]), field


def test_set_volume_round_trips_and_keeps_the_planes_not_given(gpu_ctx):
    D, W, Cc, _ = _field("33x17x9_noise_special")
    with _Volume(gpu_ctx, D, W, Cc) as ctx:
        got = ctx.tsdf_volume()
        assert got["D"].tobytes() == D.tobytes() and got["W"].tobytes() == W.tobytes() and got["C"].tobytes() == Cc.tobytes()
        W2 = np.ones_like(W)
        ctx.tsdf_set_volume(W=W2)
        got = ctx.tsdf_volume()
        assert got["D"].tobytes() == D.tobytes() and got["W"].tobytes() == W2.tobytes() and got["C"].tobytes() == Cc.tobytes()
        _same_mesh(ctx.tsdf_mesh(), mr.mesh(mr.volume(D, W2, Cc, ORIGIN, VOXEL)), "after a new W")


def test_counts_only_and_capacities(gpu_ctx):
    D, W, Cc, want = _field("33x17x9_noise_unknown")
    nv, nf = want["n_vertices"], want["n_faces"]
    assert nv > 1000 and nf > 1000
    with _Volume(gpu_ctx, D, W, Cc) as ctx:
        only = ctx.tsdf_mesh(vertices=False, faces=False)
        assert only == dict(n_vertices=nv, n_faces=nf)
        for vcap, fcap in ((nv, nf), (0, nf), (nv, 0), (nv - 1, nf), (nv, nf - 1), (nv - 1, nf - 1), (1, 1), (64, 257), (nv + 7, nf + 9)):
            vbuf = np.frombuffer(bytes([0xAB]) * (32 * (vcap + 3)), capi.Point).copy()
            fbuf = np.frombuffer(bytes([0x5A]) * (12 * (fcap + 3)), capi.Face).copy()
            got = ctx.tsdf_mesh(vertex_cap=vcap, face_cap=fcap, out=dict(vertex_buffer=vbuf, face_buffer=fbuf))
            _same_mesh(got, want, f"caps {vcap}, {fcap}", vcap, fcap)
            assert np.all(vbuf[min(vcap, nv):].view(np.uint8) == 0xAB), f"caps {vcap}, {fcap}: vertex records beyond the capacity or the count were written"
            assert np.all(fbuf[min(fcap, nf):].view(np.uint8) == 0x5A), f"caps {vcap}, {fcap}: face records beyond the capacity or the count were written"
        some = ctx.tsdf_mesh(vertices=False)
        assert "vertices" not in some
        _same_mesh(some, want, "faces alone")


def test_device_variant(gpu_ctx):
    import torch
    D, W, Cc, want = _field("33x17x9_noise_unknown")
    nv, nf = want["n_vertices"], want["n_faces"]
    with _Volume(gpu_ctx, D, W, Cc) as ctx:
        for vcap, fcap in ((nv + 5, nf + 5), (nv - 1, nf - 1)):
            verts = torch.full((vcap + 5, 32), 0xAB, dtype=torch.uint8, device="cuda")
            faces = torch.full((fcap + 5, 12), 0x5A, dtype=torch.uint8, device="cuda")
            counts = torch.zeros(2, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.tsdf_mesh_device(d_vertices=verts.data_ptr(), vertex_cap=vcap, d_faces=faces.data_ptr(), face_cap=fcap, d_n_vertices=counts.data_ptr(),
                                 d_n_faces=counts.data_ptr() + 4)
            ctx.synchronize()
            rv, rf, cn = verts.cpu().numpy(), faces.cpu().numpy(), counts.cpu().numpy()
            got = dict(n_vertices=int(cn[0]), n_faces=int(cn[1]), vertices=rv.view(capi.Point).reshape(-1)[:min(nv, vcap)],
                       faces=rf.view(capi.Face).reshape(-1)[:min(nf, fcap)])
            _same_mesh(got, want, "device variant", vcap, fcap)
            assert np.all(rv[min(nv, vcap):] == 0xAB) and np.all(rf[min(nf, fcap):] == 0x5A)
        # counts only, into device memory
        counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.tsdf_mesh_device(d_n_vertices=counts.data_ptr(), d_n_faces=counts.data_ptr() + 4)
        ctx.synchronize()
        assert counts.cpu().numpy().tolist() == [nv, nf]
        L = capi.load_library()
        before = (verts.cpu().numpy().copy(), faces.cpu().numpy().copy())
        for args, msg in (((C.c_void_p(verts.data_ptr() + 8), 4, None, 0, None, None), "tsdf: the vertex buffer must be 16-byte aligned"),
                          ((None, 0, C.c_void_p(faces.data_ptr() + 2), 4, None, None), "tsdf: the face buffer must be 4-byte aligned"),
                          ((None, 0, None, 0, C.c_void_p(counts.data_ptr() + 2), None), "tsdf: the counts must be 4-byte aligned"),
                          ((None, 0, None, 0, None, C.c_void_p(counts.data_ptr() + 1)), "tsdf: the counts must be 4-byte aligned")):
            assert L.cspm_tsdf_mesh_device(ctx.p, *args) == ERR_ARG and L.cspm_last_error(ctx.p).decode() == msg
        ctx.synchronize()
        assert np.array_equal(verts.cpu().numpy(), before[0]) and np.array_equal(faces.cpu().numpy(), before[1])
        assert counts.cpu().numpy().tolist() == [nv, nf]


INTEGRATED = ("65x5x2_65x5_K2", "33x17x9_130x67_K3_n1_all_c0.0", "96x96x64_130x67_K2")


@pytest.mark.parametrize("name", INTEGRATED)
def test_integrated_views_against_the_one_shot_entry_and_the_restatement(gpu_ctx, name):
    case = tc.BY_NAME[name]
    want = mr.mesh(case.reference()["vol"])
    if name != INTEGRATED[0]:
        assert want["n_faces"] > 100 and want["unknown_cells"] > 0
    views = case.views()
    one = capi.tsdf_mesh_depth_maps(views, case.w, case.h, case.origin, case.voxel, case.dims, **case.params)
    _same_mesh(one, want, name + ", one-shot")
    ctx = gpu_ctx
    ctx.fuse_begin(case.w, case.h, len(views))
    try:
        ctx.tsdf_begin(case.origin, case.voxel, case.dims, **case.params)
        try:
            for k, v in enumerate(views):
                ctx.fuse_push_maps(v["depth"], v["f"], v["cx"], v["cy"], v["R"], v["t"], normal=v.get("normal"), bgr=v.get("bgr"))
                ctx.tsdf_integrate(k)
                if k == 0:  # a mesh call between two integrations: the second call below sees the further views
                    first = ctx.tsdf_mesh()
                    vol0 = tr.new_volume(case.origin, case.voxel, case.dims, **case.params)
                    tr.integrate(vol0, views[0], case.w, case.h)
                    _same_mesh(first, mr.mesh(vol0), name + ", after the first view")
            _same_mesh(ctx.tsdf_mesh(), want, name + ", context")
        finally:
            ctx.tsdf_end()
    finally:
        ctx.fuse_end()


def _msg(ctx):
    return capi.load_library().cspm_last_error(ctx.p if ctx is not None else None).decode()


def test_memory_timing_and_errors():
    L = capi.load_library()
    ctx = capi.StereoContext(0)
    D, W, Cc, want = _field("65x3x2")
    nvox = D.size
    nb = -(-nvox // 256)
    nv, nf = C.c_uint(0xABABABAB), C.c_uint(0xCDCDCDCD)
    pts = np.frombuffer(bytes([0xAB]) * (32 * 8), capi.Point).copy()
    tri = np.frombuffer(bytes([0x5A]) * (12 * 8), capi.Face).copy()
    fp = C.POINTER(C.c_float)
    try:
        first = "tsdf: cspm_tsdf_begin first"
        for call in (lambda: L.cspm_tsdf_mesh(ctx.p, capi._vp(pts), 8, capi._vp(tri), 8, C.byref(nv), C.byref(nf)),
                     lambda: L.cspm_tsdf_mesh_device(ctx.p, None, 0, None, 0, None, None),
                     lambda: L.cspm_tsdf_set_volume(ctx.p, D.ctypes.data_as(fp), None, None)):
            assert call() == ERR_STATE and _msg(ctx) == first
        assert nv.value == 0xABABABAB and nf.value == 0xCDCDCDCD and np.all(pts.view(np.uint8) == 0xAB) and np.all(tri.view(np.uint8) == 0x5A)
        assert L.cspm_tsdf_mesh(None, None, 0, None, 0, None, None) == ERR_ARG and L.cspm_tsdf_set_volume(None, None, None, None) == ERR_ARG
        assert L.cspm_tsdf_mesh_device(None, None, 0, None, 0, None, None) == ERR_ARG
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == 0
        ctx.tsdf_begin(ORIGIN, VOXEL, D.shape[::-1])
        base = 12 * nvox + 4 * (nb + 1)
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == base
        ctx.tsdf_set_volume(D, W, Cc)
        ctx.tsdf_points()
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == base  # the feature unused: nothing new is allocated
        ctx.synchronize()
        ctx.enable_timing(True)
        ctx.reset_timing()
        _same_mesh(ctx.tsdf_mesh(), want, "first call")
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, nvox) and t["post"]["launches"] == 0
        ctx.enable_timing(False)
        grown = base + 4 * nvox + 4 * (nb + 1)  # first[] and the face counts
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == grown
        _same_mesh(ctx.tsdf_mesh(), want, "second call")
        ctx.tsdf_mesh(vertices=False, faces=False)
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == grown
        # all outputs NULL is a valid call
        assert L.cspm_tsdf_mesh(ctx.p, None, 0, None, 0, None, None) == 0
        ctx.tsdf_end()
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == 0
        assert L.cspm_tsdf_mesh(ctx.p, None, 0, None, 0, C.byref(nv), C.byref(nf)) == ERR_STATE and _msg(ctx) == first
        # a new volume of another size meshes with arrays of its own
        D2, W2, C2, want2 = _field("257x2x2")
        ctx.tsdf_begin(ORIGIN, VOXEL, D2.shape[::-1])
        ctx.tsdf_set_volume(D2, W2, C2)
        _same_mesh(ctx.tsdf_mesh(), want2, "a second volume")
    finally:
        ctx.close()  # with the volume and the mesh arrays still there: cspm_destroy frees them


def test_one_shot_errors_leave_the_outputs_alone():
    case = tc.BY_NAME["3x2x2_7x5_K2"]
    views = case.views()
    with pytest.raises(capi.CspmError, match="tsdf: nx, ny and nz must be at least 1"):
        capi.tsdf_mesh_depth_maps(views, case.w, case.h, case.origin, case.voxel, (3, 0, 2))
    with pytest.raises(capi.CspmError, match="fusion: the number of views must be in 1 .. 64"):
        capi.tsdf_mesh_depth_maps([], case.w, case.h, case.origin, case.voxel, case.dims)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_mesh_of_a_batch_list(gpu_ctx, tmp_path):
    """cspm_main --tsdf_mesh_ply (with and without --tsdf_ply) on three pairs == the C-ABI path on the same files, byte for byte"""
    from test_gpu_tsdf import _cli_inputs, _pair_views
    inp = _cli_inputs(tmp_path)
    mesh_ply, pts_ply, alone_ply = tmp_path / "mesh.ply", tmp_path / "points.ply", tmp_path / "alone.ply"
    res = subprocess.run(inp["base"] + [f"--fuse_ply={tmp_path / 'fused.ply'}", f"--tsdf_ply={pts_ply}", f"--tsdf_mesh_ply={mesh_ply}", "--fuse_right=true"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "TSDF: 6 views" in res.stdout and "TSDF mesh: 6 views" in res.stdout, res.stdout + res.stderr
    res = subprocess.run(inp["base"] + [f"--fuse_ply={tmp_path / 'fused.ply'}", f"--tsdf_mesh_ply={alone_ply}", "--fuse_right=true"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "TSDF mesh: 6 views" in res.stdout and "TSDF: 6 views" not in res.stdout, res.stdout + res.stderr
    ctx = gpu_ctx
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    views = []
    for k in range(3):
        views += _pair_views(ctx, k, inp, inp["poses"][k], True)
    want = capi.tsdf_mesh_depth_maps(views, inp["w"], inp["h"], **inp["vol"])
    v, f = want["vertices"], want["faces"]
    print("command line: vertices", want["n_vertices"], "faces", want["n_faces"])
    assert want["n_faces"] > 100
    vrec = np.zeros(len(v), np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)]))
    vrec["p"] = np.stack([v["x"], v["y"], v["z"]], 1)
    nrm = np.stack([v["nx"], v["ny"], v["nz"]], 1)
    nrm[np.isnan(nrm).any(1)] = 0.0
    vrec["n"] = nrm
    vrec["rgb"] = np.stack([v["r"], v["g"], v["b"]], 1)
    frec = np.zeros(len(f), np.dtype([("k", "u1"), ("v", "<i4", 3)]))
    frec["k"] = 3
    frec["v"] = f["v"]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
            "property float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(v), len(f))).encode()
    data = open(mesh_ply, "rb").read()
    assert data == head + vrec.tobytes() + frec.tobytes()
    assert open(alone_ply, "rb").read() == data
    # the vertex block is --tsdf_ply's
    body = open(pts_ply, "rb").read().partition(b"end_header\n")[2]
    assert body == vrec.tobytes()


def test_a_context_that_meshes_computes_the_same(small_pair):
    """planes and maps of a PatchMatch run are byte-identical without a volume and with a volume that is meshed around it"""
    D, W, Cc, want = _field("33x17x9_noise")
    res = []
    for mesh in (False, True):
        ctx = capi.StereoContext(0)
        try:
            if mesh:
                nz, ny, nx = D.shape
                ctx.tsdf_begin(ORIGIN, VOXEL, (nx, ny, nz))
                ctx.tsdf_set_volume(D, W, Cc)
                _same_mesh(ctx.tsdf_mesh(), want, "before the run")
            ctx.set_images(small_pair["l"], small_pair["r"])
            ctx.build_cost_grd(small_pair["max_dis"], 9, 3, 0.3)
            ctx.patchmatch(2, seed=7)
            planes = [ctx.get_planes(v) for v in (0, 1)]
            maps = ctx.postprocess_f64(valid=True)
            if mesh:
                _same_mesh(ctx.tsdf_mesh(), want, "behind the run")
                ctx.tsdf_end()
            res.append((planes, maps))
        finally:
            ctx.close()
    (pa, ma), (pb, mb) = res
    for v in (0, 1):
        assert pa[v][0].tobytes() == pb[v][0].tobytes() and pa[v][1].tobytes() == pb[v][1].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ma, mb))
