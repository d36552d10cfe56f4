"""A numpy restatement of the surface formulas (audio2photoreal_amd/surface.py, the reference's visualize/ca_body/utils/geom.py),
written from the mathematics.  Test infrastructure: the yardstick of tests/test_surface_hip.py and tests/test_surface_cpu.py, and
what tests/golden/make_golden_surface.py measures the reference's own float32 error against.

Every numeric function takes `dtype` (float64 by default): all inputs are cast to it and every operation runs in it.  The float32
run against the float64 run is the rounding error float32 arithmetic makes on a mesh: the allowance of the GPU tests for shapes
that are not in the fixture.

A surface is a dict of arrays: vi [F, 3] vertex indices, vt [T, 2] texture coordinates, vti [F, 3] texture indices, n_verts."""
import numpy as np


def nerr(got, want):
    """Normalised error of an output: max |got - want| / max |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------ normals, view cosine
def face_normals(verts, vi, dtype=np.float64, eps=1e-5):
    """[N, F, 3]: cross(p1 - p0, p2 - p0) divided by its length; a length below eps counts as 1."""
    p = np.asarray(verts, dtype)[:, np.asarray(vi)]
    n = np.cross(p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0]).astype(dtype)
    length = np.sqrt((n * n).sum(-1, keepdims=True))
    length[length < dtype(eps)] = 1
    return n / length


def vert_normals(verts, vi, dtype=np.float64, eps=1e-5):
    """[N, V, 3]: the normalised face normals summed per vertex in (face, corner) order, then the same length rule."""
    verts, vi = np.asarray(verts, dtype), np.asarray(vi)
    fn = face_normals(verts, vi, dtype, eps)
    out = np.zeros_like(verts)
    flat = vi.reshape(-1)
    contrib = np.repeat(fn, 3, axis=1)                                        # [N, 3 F, 3]: entry 3 f + k is face f
    for n in range(verts.shape[0]):
        np.add.at(out[n], flat, contrib[n])                                   # unbuffered: applied in index order
    length = np.sqrt((out * out).sum(-1, keepdims=True))
    length[length < dtype(eps)] = 1
    return out / length


def _normalize(x, dtype):
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), dtype(1e-12))


def view_cos(verts, vi, camera_pos, dtype=np.float64):
    """[N, V]: normalize(vert_normals) . normalize(verts - camera); camera_pos [N, 3] or [1, 3]."""
    verts = np.asarray(verts, dtype)
    a = _normalize(vert_normals(verts, vi, dtype), dtype)
    d = _normalize(verts - np.asarray(camera_pos, dtype).reshape(-1, 1, 3), dtype)
    return a[..., 0] * d[..., 0] + a[..., 1] * d[..., 1] + a[..., 2] * d[..., 2]


# ------------------------------------------------------------------------------------------------ UV maps
def to_uv(values, index_image, bary_image, dtype=np.float64):
    """values [N, V, C] -> [N, C, H, H]: b0 x[i0] + b1 x[i1] + b2 x[i2] where all three indices differ from -1, else 0."""
    values, idx, bary = np.asarray(values, dtype), np.asarray(index_image), np.asarray(bary_image, dtype)
    valid = (idx != -1).all(-1)
    safe = np.where(valid[..., None], idx, 0)
    x = values[:, safe]                                                       # [N, H, H, 3, C]
    out = bary[None, :, :, 0, None] * x[:, :, :, 0] + bary[None, :, :, 1, None] * x[:, :, :, 1]
    out = out + bary[None, :, :, 2, None] * x[:, :, :, 2]
    out = np.where(valid[None, :, :, None], out, dtype(0))
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def from_uv(values_uv, vt, v2uv, dtype=np.float64):
    """values_uv [N, C, H', W'] -> [N, V, C]: bilinear samples (align_corners, zero padding) at the texture coordinates of a
    vertex's 4 slots, summed in slot order and divided by 4.  Taps nw, ne, sw, se in that order."""
    x_uv, vt = np.asarray(values_uv, dtype), np.asarray(vt, dtype)
    N, C, Hs, Ws = x_uv.shape
    g = vt * dtype(2) - dtype(1)
    x = ((g[:, 0] + dtype(1)) / dtype(2)) * dtype(Ws - 1)
    y = ((g[:, 1] + dtype(1)) / dtype(2)) * dtype(Hs - 1)
    xw, yn = np.floor(x), np.floor(y)
    w, n = x - xw, y - yn
    e, s = dtype(1) - w, dtype(1) - n
    sample = np.zeros((N, C, vt.shape[0]), dtype)
    for dy, dx, wt in ((0, 0, s * e), (0, 1, s * w), (1, 0, n * e), (1, 1, n * w)):
        xi, yi = xw + dx, yn + dy
        ok = (xi >= 0) & (xi <= Ws - 1) & (yi >= 0) & (yi <= Hs - 1)
        xs, ys = np.where(ok, xi, 0).astype(np.int64), np.where(ok, yi, 0).astype(np.int64)
        sample = sample + np.where(ok, x_uv[:, :, ys, xs], dtype(0)) * wt
    slots = sample[:, :, np.asarray(v2uv)]                                    # [N, C, V, 4]
    out = ((slots[..., 0] + slots[..., 1]) + slots[..., 2]) + slots[..., 3]
    return np.ascontiguousarray((out / dtype(4)).transpose(0, 2, 1))


def bary_coords(points, triangles, dtype=np.float64, eps=1e-6):
    """points [M, 2], triangles [3, M, 2] -> [3, M]: barycentrics of each point in its triangle; the denominator is kept at
    least eps away from 0, on its own side."""
    p, t = np.asarray(points, dtype), np.asarray(triangles, dtype)
    x, x1, x2 = p[:, 0] - t[2, :, 0], t[0, :, 0] - t[2, :, 0], t[1, :, 0] - t[2, :, 0]
    y, y1, y2 = p[:, 1] - t[2, :, 1], t[0, :, 1] - t[2, :, 1], t[1, :, 1] - t[2, :, 1]
    denom = y2 * x1 - y1 * x2
    n0, n1 = y2 * x - x2 * y, x1 * y - y1 * x
    denom = np.where(denom >= 0, np.maximum(denom, dtype(eps)), np.minimum(denom, dtype(-eps)))
    b0, b1 = n0 / denom, n1 / denom
    return np.stack([b0, b1, dtype(1) - b0 - b1])


def texel_centres(H, dtype=np.float64):
    """[H] coordinates (k + 0.5) / H of the texel centres along one axis."""
    return (np.arange(H).astype(dtype) + dtype(0.5)) / dtype(H)


def raster_uv(surf_vt, vti, H, flip_uv=False, dtype=np.float64):
    """[H, H] face index image (-1: no face).  The texel at row i, column j has centre ((j + 0.5) / H, (i + 0.5) / H); a face covers
    it when the centre is inside or on the boundary of its UV triangle; a zero-area triangle covers nothing; the lowest face wins."""
    vt = np.asarray(surf_vt, dtype).copy()
    if flip_uv:
        vt[:, 1] = dtype(1) - vt[:, 1]
    c = texel_centres(H, dtype)
    out = np.full((H, H), -1, np.int64)
    for f in range(len(vti) - 1, -1, -1):                                     # descending: a lower face overwrites
        a, b, d = vt[vti[f, 0]], vt[vti[f, 1]], vt[vti[f, 2]]
        area = (b[0] - a[0]) * (d[1] - a[1]) - (b[1] - a[1]) * (d[0] - a[0])
        if area == 0:
            continue
        lo, hi = np.minimum(np.minimum(a, b), d), np.maximum(np.maximum(a, b), d)
        js, is_ = np.nonzero((c >= lo[0]) & (c <= hi[0]))[0], np.nonzero((c >= lo[1]) & (c <= hi[1]))[0]
        if not js.size or not is_.size:
            continue
        px, py = c[js][None, :], c[is_][:, None]
        w = [(q[0] - p[0]) * (py - p[1]) - (q[1] - p[1]) * (px - p[0]) for p, q in ((a, b), (b, d), (d, a))]
        inside = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
        block = out[is_[0]:is_[-1] + 1, js[0]:js[-1] + 1]
        block[inside] = f
    return out


def uv_images(surf, H, flip_uv=False, dtype=np.float64):
    """(index_image [H, H, 3] int64, bary_image [H, H, 3], face_index_image [H, H] int64) of a surface by the rule of raster_uv and
    bary_coords at the texel centres; texels without a face hold -1 / 0."""
    vi, vti = np.asarray(surf["vi"]), np.asarray(surf["vti"])
    vt = np.asarray(surf["vt"], dtype).copy()
    if flip_uv:
        vt[:, 1] = dtype(1) - vt[:, 1]
    face = raster_uv(surf["vt"], vti, H, flip_uv, dtype)
    hit = face >= 0
    safe = np.where(hit, face, 0)
    index = np.where(hit[..., None], vi[safe], -1)
    c = texel_centres(H, dtype)
    pts = np.stack(np.broadcast_arrays(c[None, :], c[:, None]), -1).reshape(-1, 2)
    tri = vt[vti[safe.reshape(-1)]].transpose(1, 0, 2)                        # [3, H H, 2]
    bary = bary_coords(pts, tri, dtype).T.reshape(H, H, 3)
    bary = np.where(hit[..., None], bary, dtype(0))
    return index.astype(np.int64), bary, face


# ------------------------------------------------------------------------------------------------ host tables
def compute_v2uv(n_verts, vi, vti, n_max=4):
    """[n_verts, n_max] int32: the sorted distinct texture indices of each vertex, unused slots holding the first one."""
    owned = [set() for _ in range(n_verts)]
    for v, t in zip(np.asarray(vi).reshape(-1), np.asarray(vti).reshape(-1)):
        owned[int(v)].add(int(t))
    out = np.zeros((n_verts, n_max), np.int32)
    for v in range(n_verts):
        vals = sorted(owned[v])
        assert 1 <= len(vals) <= n_max, (v, vals)
        out[v] = vals[0]
        out[v, :len(vals)] = vals
    return out


def incidence(n_verts, vi):
    """(inc_ptr [V + 1], inc_face): the faces of vertex v are inc_face[inc_ptr[v]:inc_ptr[v + 1]], ascending in the face and then
    the corner; a face that lists a vertex twice appears twice."""
    lists = [[] for _ in range(n_verts)]
    for f, face in enumerate(np.asarray(vi)):
        for v in face:
            lists[int(v)].append(f)
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return ptr, np.asarray([f for l in lists for f in l], np.int64)


# ------------------------------------------------------------------------------------------------ the fixture mesh
NX, NY = 23, 19            # vertex grid: 437 vertices, 22 x 18 x 2 = 792 triangles (neither a multiple of 64)
SEAM, SLIT_ROW, SLIT_END = 11, 9, 16
FAN, FOUR = (17, 4), (5, 5)
UV_SIZES = (48, 130)
EDGE_CLEARANCE = 1e-4


def uv_area(vt, vti):
    """[F]: twice the signed area of each UV triangle."""
    a, b, c = (np.asarray(vt, np.float64)[np.asarray(vti)[:, k]] for k in range(3))
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def edge_clearance(vt, vti, sizes=UV_SIZES, edges=None):
    """The smallest distance (UV units) between a texel centre of any of `sizes` and an edge of a UV triangle with area."""
    vt = np.asarray(vt, np.float64)
    if edges is None:
        t = np.asarray(vti)[uv_area(vt, vti) != 0]
        edges = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0)
    best = np.inf
    for H in sizes:
        c = texel_centres(H)
        for a, b in vt[np.asarray(edges)].reshape(-1, 2, 2):
            lo, hi = np.minimum(a, b) - 2 * EDGE_CLEARANCE, np.maximum(a, b) + 2 * EDGE_CLEARANCE
            px, py = c[(c >= lo[0]) & (c <= hi[0])][None, :], c[(c >= lo[1]) & (c <= hi[1])][:, None]
            if not px.size or not py.size:
                continue
            ab = b - a
            t = np.clip(((px - a[0]) * ab[0] + (py - a[1]) * ab[1]) / (ab @ ab), 0, 1)
            best = min(best, float(np.sqrt((px - a[0] - t * ab[0]) ** 2 + (py - a[1] - t * ab[1]) ** 2).min()))
    return best


def make_surface(seed=3):
    """The fixture mesh as data: {"vi", "vt", "vti", "n_verts", "rest"} (rest [V, 3] float32 vertex positions).

    A 23 x 19 grid with jittered heights, two triangles per quad.  The UV layout is two charts cut along column 11; the right chart
    has a slit along row 9 up to column 16, so seam vertices own 2 texture indices and the slit's root (11, 9) owns 3.  Vertex
    (5, 5) gets a private texture copy in three of its faces and owns 4.  64 faces spread over the mesh have one corner moved to
    the fan vertex (17, 4), which then sits in 70 face corners; their UV triangles collapse to the fan's texture point (zero
    area: they cover nothing), which adds that texture index to the two vertices they keep.  Every UV corner is jittered; a corner
    whose edges pass within EDGE_CLEARANCE of a texel centre at one of UV_SIZES is drawn again, so that the inside-or-on-boundary
    rule, a strict rule and float32 against float64 cannot disagree on any texel.  Asserted here: that clearance, face normal
    lengths above 1e-3 and vertex normal sums above 1e-2."""
    rs = np.random.RandomState(seed)
    vid = lambda i, j: j * NX + i
    V = NX * NY
    ii, jj = np.meshgrid(np.arange(NX), np.arange(NY))
    rest = np.stack([ii * 0.1, jj * 0.1, 0.15 * np.sin(ii * 0.4) * np.cos(jj * 0.3) + rs.randn(NY, NX) * 0.02], -1)
    rest = rest.reshape(V, 3).astype(np.float32)

    # texture points: one per (vertex, region); regions 0 = left chart, 1 = right chart below the slit, 2 = above it
    tex, pos = {}, []

    def tid(i, j, region):
        if region == 2 and not (j == SLIT_ROW and i <= SLIT_END):
            region = 1                                                        # only the slit's vertices are doubled
        key = (i, j, region)
        if key not in tex:
            u = 0.03 + 0.04 * i if region == 0 else 0.53 + 0.04 * (i - SEAM)
            v = 0.04 + 0.05 * j + (0.004 * (SLIT_END + 1 - i) if region == 2 else 0.0)
            tex[key] = len(pos)
            pos.append([u, v])
        return tex[key]

    vi, vti = [], []
    for qj in range(NY - 1):
        for qi in range(NX - 1):
            region = 0 if qi < SEAM else (1 if qj < SLIT_ROW else 2)
            c = [(qi, qj), (qi + 1, qj), (qi + 1, qj + 1), (qi, qj + 1)]
            for tri in ((0, 1, 2), (0, 2, 3)):
                vi.append([vid(*c[k]) for k in tri])
                vti.append([tid(*c[k], region) for k in tri])
    vi, vti = np.asarray(vi, np.int64), np.asarray(vti, np.int64)
    F = len(vi)
    assert (V, F) == (437, 792)
    pos = np.asarray(pos)
    cell = np.array([0.04, 0.05])
    base = pos.copy()

    # the vertex with 4 texture indices: a private copy, pulled towards the face's centroid, in three of its faces
    four = vid(*FOUR)
    faces4 = np.nonzero((vi == four).any(1))[0][:3]
    for f in faces4:
        k = int(np.nonzero(vi[f] == four)[0][0])
        base = np.vstack([base, 0.8 * base[vti[f, k]] + 0.2 * base[vti[f]].mean(0)])
        vti[f, k] = len(base) - 1

    # the fan: 64 faces away from the seam, the slit, the 4-index vertex and the fan's own ring give it one corner each
    fan = vid(*FAN)
    t_fan = tex[(FAN[0], FAN[1], 1)]
    ring = lambda f, centre, r: np.abs(np.array([[v % NX, v // NX] for v in vi[f]]) - np.array(centre)).max() <= r
    free = [f for f in range(F) if f not in faces4 and not ring(f, FAN, 2) and not ring(f, FOUR, 2)
            and all(abs(v % NX - SEAM) > 1 for v in vi[f]) and not (vi[f].max() // NX >= SLIT_ROW - 1 and vi[f].min() // NX <= SLIT_ROW + 1
                                                                   and vi[f].min() % NX >= SEAM)]
    for f in rs.choice(free, size=64, replace=False):
        vi[f, 0] = fan
        vti[f] = t_fan
        e1, e2 = rest[vi[f, 1]] - rest[fan], rest[vi[f, 2]] - rest[fan]
        if np.cross(e1, e2)[2] < 0:                                           # keep every normal on the grid's side
            vi[f, [1, 2]] = vi[f, [2, 1]]
    assert int((vi == fan).sum()) == 70

    # jitter every UV corner; draw again while one of its edges passes too close to a texel centre
    t = vti[uv_area(base, vti) != 0]
    edges = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0)
    vt = (base + rs.uniform(-0.12, 0.12, base.shape) * cell).astype(np.float32).astype(np.float64)
    mine = [edges[(edges == k).any(1)] for k in range(len(vt))]
    for _ in range(50):                                                       # sweeps: a corner may wait for a neighbour to move
        moved = False
        for k in range(len(vt)):
            for _ in range(20):
                if not len(mine[k]) or edge_clearance(vt, vti, edges=mine[k]) > 2 * EDGE_CLEARANCE:
                    break
                vt[k] = np.float32(base[k] + rs.uniform(-0.12, 0.12, 2) * cell)
                moved = True
        if not moved:
            break
    vt = vt.astype(np.float32)

    surf = {"vi": vi, "vt": vt, "vti": vti, "n_verts": V, "rest": rest}
    assert edge_clearance(vt, vti) > EDGE_CLEARANCE
    p = rest.astype(np.float64)[vi]
    assert np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).min() > 1e-3
    counts = sorted(len(set(r)) for r in compute_v2uv(V, vi, vti))
    assert counts[-1] == 4 and counts[-2] == 3 and counts.count(4) == 1
    return surf


def make_frames(surf, seed, N):
    """[N, V, 3] float32: the rest positions bent and jittered per frame; asserts the normal sums stay above 1e-2."""
    rs = np.random.RandomState(seed)
    rest = surf["rest"].astype(np.float64)
    out = []
    for n in range(N):
        p = rest.copy()
        p[:, 2] += 0.1 * np.sin(rest[:, 0] * (1.0 + 0.3 * n) + n) + rs.randn(len(p)) * 0.01
        p[:, :2] += rs.randn(len(p), 2) * 0.005
        out.append(p)
    verts = np.asarray(out, np.float32)
    fn = face_normals(verts, surf["vi"])
    sums = np.zeros(verts.shape)
    for n in range(N):
        np.add.at(sums[n], surf["vi"].reshape(-1), np.repeat(fn[n], 3, axis=0))
    p = verts.astype(np.float64)[:, surf["vi"]]
    assert np.linalg.norm(np.cross(p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0]), axis=-1).min() > 1e-3
    assert np.linalg.norm(sums, axis=-1).min() > 1e-2
    return verts
