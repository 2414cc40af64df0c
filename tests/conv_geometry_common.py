"""Sparse convolutions at every kernel geometry: the case table, a float64 dense-conv3d reference, brute-force integer
tables and the per-element comparator that tests/test_conv_geometry.py (CPU) and tests/test_gpu_conv_geometry.py share.
numpy / torch-CPU only: nothing here touches the GPU or the library.

REFERENCE.  A sparse convolution is a dense one restricted to active sites: scatter the rows into a float64
[B, Cin, D, H, W] tensor, run torch.nn.functional.conv3d with the weight [kD,kH,kW,Cin,Cout] permuted to
[Cout,Cin,kD,kH,kW], and read the active outputs.  Strided convs use their stride and padding, and an output is active
where the same conv of the occupancy mask with a ones-kernel is positive; SubM convs use stride 1 and padding ks // 2,
cropped to [:D,:H,:W] (an even kernel's taps are asymmetric: offsets -ks/2 .. ks/2 - 1) and read at the input sites.
dX and dW come from autograd.  A second pass on |x|, |w| (|g|) gives S, each element's sum of absolute products.

VALUES.  Features, weights and output gradients have magnitudes uniform in [1/2, 1] with random sign, so a single product
is at least 1/4 and, with 4 n c(n) < 1, one missing or misplaced product moves an element by more than its bound.

COMPARATOR.  Per element |got - ref| <= c(n) S with c(n) = (3 n + 16) 2^-24, n the element's number of products
(K Cin forward, K Cout for dX, the tap's pair count for dW):
  3 n   the accumulation bound tests/split_model.py states for the three-product f16x3 sum (hi hi + hi lo + lo hi, each
        added in fp32 with unit roundoff 2^-24: three additions per product);
  12    both operands travel as a 22-bit hi + lo pair (2 x 2^-22 = 8 units of 2^-24 on a product) and the lo lo term is
        dropped (2^-22 = 4 units);
  4     the result is stored as split rows (2^-22).
The fp32 kernels (one rounding per product and per addition: 2 n 2^-24) sit below it.  Where S == 0 (taps no pair uses,
input rows that feed no output) the result must be exactly 0.  The bound is derived, not fitted to any kernel's output."""
import functools
import itertools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
MAX_N = 1179          # 4 n c(n) < 1  <=>  n <= 1179
MAX_ROWS = 1100

# (kernel, stride, padding) of the strided convs
STRIDED = [
    ((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)), ((3, 3, 3), (1, 1, 1), (1, 1, 1)),
    ((3, 3, 3), (1, 1, 1), (0, 0, 0)), ((3, 3, 3), (3, 2, 1), (1, 1, 0)), ((3, 1, 1), (2, 1, 1), (0, 0, 0)),
    ((2, 2, 2), (2, 2, 2), (0, 0, 0)), ((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((1, 1, 1), (2, 2, 2), (0, 0, 0)),
    ((1, 3, 3), (1, 2, 2), (0, 1, 1)), ((3, 3, 1), (3, 3, 1), (1, 0, 0)), ((5, 5, 1), (2, 1, 1), (2, 2, 0)),
    ((1, 1, 3), (1, 1, 3), (0, 0, 2)), ((2, 3, 1), (1, 2, 1), (1, 0, 0)), ((3, 3, 2), (1, 1, 1), (0, 0, 0)),
]
# SubM kernels; (1, 1, 2) is the two-tap kernel (a one-step pipeline's neighbour)
SUBM = [(3, 3, 3), (1, 1, 1), (3, 1, 1), (1, 3, 3), (1, 1, 3), (3, 3, 1), (5, 5, 1), (2, 2, 2), (3, 3, 2), (1, 1, 2)]
GRIDS = [(1, (1, 1, 1)), (1, (4, 5, 1)), (3, (3, 4, 7)), (2, (2, 3, 63)), (2, (2, 3, 64)), (1, (3, 2, 65)), (2, (9, 8, 20))]
OCCUPANCIES = ("one", "sparse", "full")
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ROW_COUNT_GRID = (2, (9, 8, 20))
K_REQUIRED = (1, 3, 6, 8, 9, 18, 25, 27)


class Geometry:
    def __init__(self, subm, ks, st=(1, 1, 1), pd=None):
        self.subm, self.ks = bool(subm), tuple(ks)
        self.st = (1, 1, 1) if subm else tuple(st)
        self.pd = tuple(k // 2 for k in ks) if subm else tuple(pd)
        self.K = int(np.prod(ks))

    @property
    def name(self):
        j = lambda t: "".join(str(v) for v in t)
        return f"subm_k{j(self.ks)}" if self.subm else f"conv_k{j(self.ks)}_s{j(self.st)}_p{j(self.pd)}"

    def out_shape(self, shape):
        if self.subm:
            return tuple(shape)
        return tuple((d + 2 * p - k) // s + 1 for d, k, s, p in zip(shape, self.ks, self.st, self.pd))

    def fits(self, shape):
        """the static drop rule: a grid narrower than the kernel (after padding) has an empty output shape"""
        return self.subm or all(d + 2 * p >= k for d, k, p in zip(shape, self.ks, self.pd))

    def has_lines(self, taps_per_line):
        """does the table have a line-compressed form of `taps_per_line` taps per line (for rows in rank order; with one tap
        per line any order)?  Lines are the kernel's x-lines (3 taps) or single taps, nine at the most."""
        if taps_per_line == 3:
            return self.ks[2] == 3 and self.ks[0] * self.ks[1] <= 9
        return self.K <= 9


GEOMETRIES = [Geometry(False, *g) for g in STRIDED] + [Geometry(True, ks) for ks in SUBM]


class Case:
    """one active set: geometry, grid, rows idx int32 [n, 4] = (b, z, y, x) in the order the convolution sees them"""

    def __init__(self, geom, batch, shape, occ, shuffled, idx):
        self.geom, self.batch, self.shape, self.occ, self.shuffled, self.idx = geom, batch, tuple(shape), occ, shuffled, idx
        self.n = idx.shape[0]

    @property
    def id(self):
        s = "x".join(str(v) for v in self.shape)
        return f"{self.geom.name}-b{self.batch}_{s}-{self.occ}-{'shuffled' if self.shuffled else 'ranked'}"

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())


def _cells(batch, shape):
    return batch * int(np.prod(shape))


def _rows(batch, shape, count, rng):
    """`count` distinct cells, (b, z, y, x)-sorted"""
    D, H, W = shape
    lin = np.sort(rng.choice(_cells(batch, shape), count, replace=False))
    return np.stack([lin // (D * H * W), lin // (H * W) % D, lin // W % H, lin % W], 1).astype(np.int32)


def occupancy_count(batch, shape, occ):
    cells = _cells(batch, shape)
    if occ == "one":
        return 1
    if occ == "sparse":
        return max(1, round(0.07 * cells))
    return cells if cells <= 1100 else round(0.3 * cells)       # "full"


def combos():
    """every geometry x grid x occupancy, dropped ones included -> (geometry, batch, shape, occupancy)"""
    return [(g, b, s, o) for g in GEOMETRIES for (b, s) in GRIDS for o in OCCUPANCIES]


def _make_cases():
    cases = []
    for g, b, s, occ in combos():
        if not g.fits(s):
            continue
        count = occupancy_count(b, s, occ)
        for shuffled in (False, True):
            if shuffled and count == 1:
                continue                  # one row has one order
            name = f"{g.name}-{b}-{s}-{occ}"
            rng = np.random.default_rng(zlib.crc32(name.encode()))
            idx = _rows(b, s, count, rng)
            if shuffled:
                idx = idx[rng.permutation(count)]
            cases.append(Case(g, b, s, occ, shuffled, np.ascontiguousarray(idx)))
    b, s = ROW_COUNT_GRID
    for g in (Geometry(True, (3, 3, 3)), Geometry(False, (3, 3, 3), (2, 2, 2), (1, 1, 1))):
        for count in ROW_COUNTS:
            for shuffled in (False, True):
                if shuffled and count == 1:
                    continue
                rng = np.random.default_rng(zlib.crc32(f"{g.name}-rows{count}".encode()))
                idx = _rows(b, s, count, rng)
                if shuffled:
                    idx = idx[rng.permutation(count)]
                cases.append(Case(g, b, s, f"rows{count}", shuffled, np.ascontiguousarray(idx)))
    return cases


CASES = _make_cases()
GROUPS = sorted({c.geom.name for c in CASES})          # one test parameter per geometry


def cases_of(group):
    return [c for c in CASES if c.geom.name == group]


# ------------------------------------------------------------------------------------------------ kernel families
# family -> channel shapes (the entries are in tests/test_gpu_conv_geometry.py)
NARROW = [(32, 32), (64, 32), (32, 64), (64, 64)]
FAMILIES = {
    "fp32_mfma": [(16, 16), (16, 32)],
    "generic": [(5, 16), (48, 80)],
    "tile": [(32, 128), (32, 256), (64, 64), (128, 32)],
    "dma": NARROW,
    "dma_lines3": NARROW,
    "dma_lines1": NARROW,
    "staged": NARROW,
    "cu": [(128, 256)],
    "best": NARROW + [(32, 128), (32, 256), (128, 32), (128, 256)],
}
BACKWARD_SPLIT = [(32, 32), (32, 64), (64, 32)]
BACKWARD_FP32 = [(16, 16), (16, 32), (5, 16), (48, 80)]


def n_ok(K, c_in, c_out, backward=False):
    """4 n c(n) < 1 for the forward pass (n = K Cin) and, for backward, dX (n = K Cout); dW's n is a pair count, bounded
    by MAX_ROWS"""
    return K * c_in <= MAX_N and (not backward or K * c_out <= MAX_N)


def family_takes(family, case, c_in, c_out):
    """the static predicate: can this family serve this case at this channel shape inside the comparator's range?"""
    g = case.geom
    if not n_ok(g.K, c_in, c_out):
        return False
    if family == "dma_lines3":
        return g.has_lines(3) and not case.shuffled
    if family == "dma_lines1":
        return g.has_lines(1)
    return True


def family_shapes(family, case):
    return [s for s in FAMILIES[family] if family_takes(family, case, *s)]


# ------------------------------------------------------------------------------------------------ values
def signed_half_to_one(rng, shape):
    """magnitudes uniform in [1/2, 1], random sign, float32"""
    return (rng.uniform(0.5, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ brute-force tables
class Tables:
    """out_idx int32 [m, 4], nbr int32 [K, m], nbr_t int32 [K, n], pairs: per tap (in rows, out rows) in output-row order"""

    def __init__(self, out_idx, nbr, nbr_t, pairs):
        self.out_idx, self.nbr, self.nbr_t, self.pairs = out_idx, nbr, nbr_t, pairs
        self.num_out = out_idx.shape[0]
        self.counts = np.array([len(p[0]) for p in pairs], np.int64)


@functools.lru_cache(maxsize=None)
def tables(case):
    g = case.geom
    rows = {tuple(int(v) for v in c): i for i, c in enumerate(case.idx)}
    assert len(rows) == case.n
    osh = g.out_shape(case.shape)
    taps = list(itertools.product(range(g.ks[0]), range(g.ks[1]), range(g.ks[2])))   # k = (kz * ks1 + ky) * ks2 + kx
    if g.subm:
        outs = [tuple(int(v) for v in c) for c in case.idx]
    else:
        seen = set()
        for (b, z, y, x) in rows:
            for kz, ky, kx in taps:
                t = (z + g.pd[0] - kz, y + g.pd[1] - ky, x + g.pd[2] - kx)
                if all(v >= 0 and v % s == 0 and v // s < o for v, s, o in zip(t, g.st, osh)):
                    seen.add((b, t[0] // g.st[0], t[1] // g.st[1], t[2] // g.st[2]))
        outs = sorted(seen)
    m = len(outs)
    nbr = np.full((g.K, m), -1, np.int32)
    nbr_t = np.full((g.K, case.n), -1, np.int32)
    for o, (b, z, y, x) in enumerate(outs):
        for k, (kz, ky, kx) in enumerate(taps):
            i = rows.get((b, z * g.st[0] - g.pd[0] + kz, y * g.st[1] - g.pd[1] + ky, x * g.st[2] - g.pd[2] + kx), -1)
            nbr[k, o] = i
            if i >= 0:
                assert nbr_t[k, i] < 0
                nbr_t[k, i] = o
    pairs = []
    for k in range(g.K):
        o = np.nonzero(nbr[k] >= 0)[0]
        pairs.append((nbr[k, o].astype(np.int32), o.astype(np.int32)))
    return Tables(np.array(outs, np.int32).reshape(m, 4), nbr, nbr_t, pairs)


# ------------------------------------------------------------------------------------------------ float64 reference
class Reference:
    """inputs x [n, Cin], w [*ks, Cin, Cout], g [m, Cout] (float32 numpy) and the float64 results out / dx / dw with their
    sums of absolute products s_out / s_dx / s_dw; out_idx int32 [m, 4] the active outputs in output-row order"""


def _dense(case, rows, channels):
    d = torch.zeros((case.batch, channels, *case.shape), dtype=torch.float64)
    i = torch.from_numpy(case.idx.astype(np.int64))
    d[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = rows
    return d


def _conv(case, xd, w):
    """dense conv3d of the case's geometry, weight [*ks, Cin, Cout]"""
    g = case.geom
    y = F.conv3d(xd, w.permute(4, 3, 0, 1, 2), stride=g.st, padding=g.pd)
    if g.subm:
        D, H, W = case.shape
        y = y[:, :, :D, :H, :W]
    return y


def active_outputs(case):
    """int64 [m, 4]: SubM: the input sites in input order; strided: where the conv of the occupancy mask with a ones-kernel
    is positive, (b, z, y, x)-sorted"""
    if case.geom.subm:
        return torch.from_numpy(case.idx.astype(np.int64))
    mask = _dense(case, torch.ones((case.n, 1), dtype=torch.float64), 1)
    hit = _conv(case, mask, torch.ones((*case.geom.ks, 1, 1), dtype=torch.float64))[:, 0] > 0.5
    return torch.nonzero(hit)                # row-major: sorted by (b, z, y, x)


def _pass(case, oi, x, w, g):
    """(out rows, dX rows, dW) of one pass through the dense conv, autograd for the gradients"""
    with torch.enable_grad():           # whatever mode the caller is in
        x = x.clone().requires_grad_(True)
        w = w.clone().requires_grad_(True)
        y = _conv(case, _dense(case, x, x.shape[1]), w)
        out = y[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]]
        (out * g).sum().backward()
    return out.detach().numpy(), x.grad.numpy(), w.grad.numpy()


@functools.lru_cache(maxsize=64)
def reference(case, c_in, c_out):
    rng = np.random.default_rng([case.seed, c_in, c_out])
    oi = active_outputs(case)
    r = Reference()
    r.out_idx = oi.numpy().astype(np.int32)
    r.x = signed_half_to_one(rng, (case.n, c_in))
    r.w = signed_half_to_one(rng, (*case.geom.ks, c_in, c_out))
    r.g = signed_half_to_one(rng, (oi.shape[0], c_out))
    x, w, g = (torch.from_numpy(a).double() for a in (r.x, r.w, r.g))
    r.out, r.dx, r.dw = _pass(case, oi, x, w, g)
    r.s_out, r.s_dx, r.s_dw = _pass(case, oi, x.abs(), w.abs(), g.abs())
    for a in (r.x, r.w, r.g, r.out, r.dx, r.dw, r.s_out, r.s_dx, r.s_dw, r.out_idx):
        a.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------------------ comparator
def c_of(n):
    return (3.0 * np.asarray(n, np.float64) + 16.0) * U24


def ratio(got, ref, S, n):
    """max over the elements of |got - ref| / (c(n) S), inf where an element with S == 0 is not exactly 0 (or got is not
    finite).  n: a number or an array that broadcasts against the result (dW: the taps' pair counts [K, 1, 1])."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    if got.size == 0:
        return 0.0
    bound = c_of(n) * S
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(S > 0, err / np.where(S > 0, bound, 1.0), np.where(got == 0, 0.0, np.inf))
    q = np.where(np.isfinite(got), q, np.inf)
    return float(q.max())


def dw_n(case):
    """n of every dW element: its tap's pair count, shaped to broadcast over [*ks, Cin, Cout]"""
    return tables(case).counts.reshape(*case.geom.ks, 1, 1)


def ratios(case, r, out=None, dx=None, dw=None):
    """{name: ratio} of the results given, against Reference r"""
    c_in, c_out = r.x.shape[1], r.g.shape[1]
    K = case.geom.K
    q = {}
    if out is not None:
        q["out"] = ratio(out, r.out, r.s_out, K * c_in)
    if dx is not None:
        q["dx"] = ratio(dx, r.dx, r.s_dx, K * c_out)
    if dw is not None:
        q["dw"] = ratio(dw, r.dw, r.s_dw, dw_n(case))
    return q


assert len({c.id for c in CASES}) == len(CASES)
