"""Inputs of the MXFP4 tests, built on the CPU so that the CPU tests can
check what the GPU tests rely on (exactness bounds, sensitivity to the K-loop
failure modes) without a kernel in the loop.  Everything is seeded."""
import functools

import numpy as np
import torch

from bodywork_mlops_demo_amd.ops import reference as ref

GRID_VALUES = (0, .5, 1, 1.5, 2, 3, 4, 6, -.5, -1, -1.5, -2, -3, -4, -6)

#: K -> the K-loop path gemm_mxfp4_nt_kernel takes (nt = K / 256 tiles)
KLOOP_PATHS = {
    256: "nt 1: single tile, no B(1) staging, first phase waits vmcnt(0)",
    512: "nt 2: no trip, two-tile tail",
    768: "nt 3: no trip, three-tile tail",
    1280: "nt 5: one trip + three-tile tail after a slot rotation",
    1536: "nt 6: two trips + two-tile tail",
    1792: "nt 7: two trips + three-tile tail, odd rotation",
}


def grid_parts(rows, seed, spread, K):
    """(grid values [rows, K], block exponents s [rows, K/32]) of
    :func:`grid_operand`."""
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor(GRID_VALUES)[torch.randint(0, 15, (rows, K), generator=g)]
    x[:, ::32] = torch.tensor([4., -6., 6., -4.])[
        torch.randint(0, 4, (rows, K // 32), generator=g)]
    row = torch.arange(rows)[:, None]
    blk = torch.arange(K // 32)[None, :]
    s = (row * spread[0] + blk * spread[1] + (row // 16) * (blk // 4)) % 3
    return x, s


def grid_operand(rows, seed, spread, K):
    """(grid value, all 15) x 2^s(row, block), s in {0,1,2}; each block holds
    a 4 or a 6, so the quantiser must choose e = s."""
    x, s = grid_parts(rows, seed, spread, K)
    return x * (2.0 ** s).repeat_interleave(32, dim=1)


@functools.lru_cache(maxsize=None)
def kloop_case(K):
    """The exact K-loop inputs at one K: a, b [512, K] fp32 and the integer
    head vectors b2, w3 [512]; fp64 references c = a.b^T and the head y.
    Products are multiples of 2^-2 and sum |a||b| stays below 2^22, so every
    partial sum in any order is exact in fp32; the same holds for the head."""
    a = grid_operand(512, 1, (1, 1), K)
    b = grid_operand(512, 2, (2, 1), K)
    c = a.double() @ b.double().t()
    bound = (a.abs().double() @ b.abs().double().t()).max().item()
    assert bound < 2 ** 22, bound  # exact in fp32 in any order
    g = torch.Generator().manual_seed(3)
    b2 = torch.randint(-8, 9, (512,), generator=g).float()
    w3 = torch.randint(-8, 9, (512,), generator=g).float()
    h2 = torch.relu(c + b2.double())
    assert (h2 * w3.double().abs()).sum(1).max() < 2 ** 22  # exact in fp32
    return dict(a=a, b=b, c=c, b2=b2, w3=w3, y=h2 @ w3.double(), bound=bound)


# ---- operands packed directly from codes and exponents ---------------------

def pack(codes, exps):
    """codes uint8 [R, K] (0..15), exps int [R, K/32] in [-127, 127] -> the
    (q, s) pair the ops take: element 2i in the low nibble of byte i, scale
    byte e + 127 at ``ref.mxfp4_scale_index``.  No quantiser involved."""
    codes = np.asarray(codes, dtype=np.uint8)
    R, K = codes.shape
    q = codes[:, 0::2] | (codes[:, 1::2] << 4)
    s = np.zeros(R * K // 32, dtype=np.uint8)
    s[ref.mxfp4_scale_index(R, K).numpy().reshape(-1)] = (
        np.asarray(exps) + 127).reshape(-1)
    return torch.from_numpy(q), torch.from_numpy(s)


def code_values(codes):
    """fp64 grid values of e2m1 codes, written out here and not taken from
    the oracle."""
    mags = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    codes = np.asarray(codes)
    return mags[codes & 7] * np.where(codes & 8, -1.0, 1.0)


def decode64(codes, exps):
    """fp64 [R, K] logical operand of (codes, exps): 6 * 2^127 is finite
    here, which it is not in fp32."""
    scale = np.exp2(np.asarray(exps, np.float64))
    return code_values(codes) * np.repeat(scale, 32, axis=1)


@functools.lru_cache(maxsize=None)
def e8m0_case(K, variant):
    """256 x 256 x K operands over the whole E8M0 range.

    ``cancel``: ea = u[row] + p[j], eb = v[col] - p[j], p uniform in
    [-125, 125], u, v in {0, 1, 2}; block 0 pinned to (-127, +127), block 1
    to (+127, -127).  Every product is a multiple of 2^-2.
    ``spread``: ea = U[row] + p[j], eb = V[col] - p[j], U, V over [-40, 40]
    (p in [-87, 87] keeps both in range): C[row, col] is an exact multiple of
    2^(U+V-2) and spans 2^+-80 across elements.
    ``free``: as ``cancel`` without the pinned blocks, but u and v drawn per
    (row, block): no two K-tiles share a scale pattern in either operand or
    in their sum, which the other inputs cannot offer at nt > 3.
    """
    rng = np.random.default_rng(
        40 + K + ("cancel", "spread", "free").index(variant))
    nb = K // 32
    ca = rng.integers(0, 16, (256, K), dtype=np.uint8)
    cb = rng.integers(0, 16, (256, K), dtype=np.uint8)
    if variant == "cancel":
        p = rng.integers(-125, 126, nb)
        u, v = rng.integers(0, 3, (2, 256, 1))
    elif variant == "free":
        p = rng.integers(-125, 126, nb)
        u, v = rng.integers(0, 3, (2, 256, nb))
    else:
        p = rng.integers(-87, 88, nb)
        u, v = rng.integers(-40, 41, (2, 256, 1))
        u[:2, 0], v[:2, 0] = (-40, 40), (-40, 40)  # both ends are present
    ea = u + p[None, :]
    eb = v - p[None, :]
    if variant == "cancel":
        ea[:, 0], eb[:, 0] = -127, 127
        ea[:, 1], eb[:, 1] = 127, -127
    assert np.abs(ea).max() <= 127 and np.abs(eb).max() <= 127
    # the reference: products of code values and of exact powers of two
    va, vb = code_values(ca), code_values(cb)
    c = np.zeros((256, 256))
    absum = np.zeros((256, 256))
    for j in range(nb):
        sl = slice(32 * j, 32 * j + 32)
        scale = np.exp2((ea[:, j][:, None] + eb[:, j][None, :]).astype(float))
        c += (va[:, sl] @ vb[:, sl].T) * scale
        absum += (np.abs(va[:, sl]) @ np.abs(vb[:, sl]).T) * scale
    unit = (np.exp2((u + v.T).astype(float) - 2) if variant == "spread"
            else np.full((256, 256), 0.25))
    # in units of the smallest product every partial sum is an integer below
    # 2^24: exact in fp32 in any order
    assert (absum / unit).max() < 2 ** 24
    assert np.array_equal(c / unit, np.round(c / unit))
    assert np.array_equal(c.astype(np.float32).astype(np.float64), c)
    return dict(ca=ca, ea=ea, cb=cb, eb=eb, c=torch.from_numpy(c),
                absum=absum.max(), aq=pack(ca, ea), bq=pack(cb, eb))


# ---- quantiser edges -------------------------------------------------------

def _successor(v, dtype):
    """the next representable value above a positive v in ``dtype``"""
    t = torch.tensor([v], dtype=dtype)
    bits = t.view(torch.int32 if dtype == torch.float32 else torch.int16)
    return (bits + 1).view(dtype).double().item()


def edge_amaxes(dtype):
    """[(label, block amax as a python float, expected scale byte)] for the
    quantiser edge tests; every value is exact in ``dtype``."""
    out = []
    if dtype == torch.float32:
        out.append(("min subnormal", 2.0 ** -149, 0))
    else:
        out.append(("min subnormal", 2.0 ** -133, 0))
    out.append(("subnormal 1.5*2^-127", 1.5 * 2.0 ** -127, 0))
    out.append(("exponent field 1", 2.0 ** -126, 0))  # e = -128 clamps
    for k in (-126, -3, 0, 120):
        top = 6.0 * 2.0 ** k
        out.append((f"6*2^{k}", top, k + 127))
        out.append((f"above 6*2^{k}", _successor(top, dtype), k + 128))
    out.append(("finfo.max", float(torch.finfo(dtype).max), 253))
    return out


@functools.lru_cache(maxsize=None)
def edge_input(dtype, K):
    """x [64, K] in ``dtype``: ordinary blocks over many binades, and every
    :func:`edge_amaxes` value as the amax of four blocks with ordinary
    smaller neighbours (at most 3/4 of it).  Returns (x, [(label, row, block,
    position, byte)])."""
    g = torch.Generator().manual_seed(11 + K)
    nb = K // 32
    x = torch.randn(64, K, generator=g, dtype=torch.float64)
    x = x * 2.0 ** torch.randint(-12, 12, (64, nb), generator=g).double(
        ).repeat_interleave(32, dim=1)
    frac = torch.rand(64, K, generator=g, dtype=torch.float64) * 1.5 - 0.75
    where = []
    slots = iter(torch.randperm(64 * nb, generator=g).tolist())  # distinct
    for i, (label, amax, byte) in enumerate(edge_amaxes(dtype)):
        for rep in range(4):
            row, blk = divmod(next(slots), nb)
            pos = (i * 7 + rep * 9) % 32
            sl = slice(32 * blk, 32 * blk + 32)
            x[row, sl] = frac[row, sl] * amax
            x[row, 32 * blk + pos] = amax if rep % 2 == 0 else -amax
            where.append((label, row, blk, pos, byte))
    x = x.to(dtype)
    amax_of = {label: amax for label, amax, _ in edge_amaxes(dtype)}
    for label, row, blk, pos, _ in where:  # the cast kept every amax
        amax = amax_of[label]
        assert abs(x[row, 32 * blk + pos].double().item()) == amax
        assert x[row, 32 * blk:32 * blk + 32].double().abs().max() == amax
    return x, where


#: fp32 bit patterns of the non-finite elements (bf16 takes the top half;
#: written as bits because a float cast may canonicalise a NaN)
NONFINITE_BITS = {
    "+inf": 0x7F800000, "-inf": 0xFF800000,
    "+nan": 0x7FC00000, "-nan": 0xFFC00000,
    "+nan payload": 0x7FEA0000, "-nan signalling": 0xFF950000,
}


def _set_bits(x, row, col, bits32):
    if x.dtype == torch.float32:
        xi, bits, width = x.view(torch.int32), bits32, 32
    else:
        xi, bits, width = x.view(torch.int16), bits32 >> 16, 16
    xi[row, col] = bits - (1 << width) if bits >> (width - 1) else bits


@functools.lru_cache(maxsize=None)
def nonfinite_input(dtype, K):
    """x [64, K] whose marked blocks hold one non-finite element (two in the
    last block) next to finite neighbours in [-6, 6], and ``twin``: the same
    with each non-finite element replaced by a 6 of its sign, which pins
    e = 0, so the twin's codes are what the neighbours must get.  Returns
    (x, twin, [(kind, row, block, position)])."""
    g = torch.Generator().manual_seed(21 + K)
    nb = K // 32
    x = (torch.randn(64, K, generator=g) * 3).clamp(-6, 6).to(dtype)
    twin = x.clone()
    where = []
    slots = iter(torch.randperm(64 * nb, generator=g).tolist())  # distinct

    def put(kind, slot, pos):
        row, blk = divmod(slot, nb)
        _set_bits(x, row, 32 * blk + pos, NONFINITE_BITS[kind])
        twin[row, 32 * blk + pos] = -6.0 if kind[0] == "-" else 6.0
        where.append((kind, row, blk, pos))

    for i, kind in enumerate(NONFINITE_BITS):
        for rep in range(8):  # every nibble of a lane's 4 bytes, every lane
            put(kind, next(slots), (rep + 8 * ((i + rep) % 4) + 3 * i) % 32)
    # a NaN and an inf in one block
    slot = next(slots)
    put("+nan", slot, 4)
    put("-inf", slot, 21)
    nonfinite = ~torch.isfinite(x.float())
    assert int(nonfinite.sum()) == len(where)
    assert int(torch.isnan(x.float()).sum()) == 4 * 8 + 1
    return x, twin, where


def nibble(q, row, k):
    """code of element k of a row of packed codes q"""
    return (int(q[row, k // 2]) >> (4 * (k % 2))) & 0xF


def unpack(q):
    """packed codes uint8 [R, K/2] -> codes uint8 [R, K]"""
    return torch.stack((q & 0xF, q >> 4), dim=2).reshape(
        q.shape[0], 2 * q.shape[1])
