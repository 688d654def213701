"""MXFP4 (e2m1 codes, per-32-element E8M0 block scales) oracle and the
fp4 scoring flag, on the CPU."""
import numpy as np
import pytest
import torch

import mx4_data
from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.ops import reference as ref

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _roundtrip(x):
    q, s = ops.quantize_mxfp4(x)
    return q, s, ref.mxfp4_decode_cpu(q, s, x.shape[1])


@pytest.mark.parametrize("k", [-20, -1, 0, 3, 40])
def test_grid_values_round_trip(k):
    """Every grid value times 2^k, both signs, comes back exactly; blocks
    that hold a 4 or a 6 and blocks that do not."""
    vals = torch.tensor(GRID + [-v for v in GRID[1:]])
    g = torch.Generator().manual_seed(k + 100)
    x = vals[torch.randint(0, 15, (64, 256), generator=g)] * 2.0 ** k
    x[:, ::64] = 6.0 * 2.0 ** k
    _, _, back = _roundtrip(x)
    assert torch.equal(back, x)


@pytest.mark.parametrize("k", [-126, -3, 0, 5, 120])
def test_exponent_rule_at_the_boundary(k):
    """amax = 6 * 2^k gives e = k, the next float above gives k + 1."""
    top = np.float32(6.0 * 2.0 ** k)
    above = np.nextafter(top, np.float32(np.inf))
    assert ref.mxfp4_block_exponent(np.array([top, above])).tolist() == [
        k, k + 1]
    x = torch.zeros(64, 256)
    x[0, 5], x[1, 40] = float(top), float(above)
    _, s, _ = _roundtrip(x)
    idx = ref.mxfp4_scale_index(64, 256)
    assert int(s[idx[0, 0]]) == k + 127 and int(s[idx[1, 1]]) == k + 128


@pytest.mark.parametrize("value, want", [
    (2.5, 2.0), (3.5, 4.0), (5.0, 4.0), (0.25, 0.0), (0.75, 1.0),
    (1.25, 1.0), (-2.5, -2.0), (-5.0, -4.0)])
def test_ties_go_to_the_even_code(value, want):
    x = torch.zeros(64, 256)
    x[:, 0] = 6.0  # pins every first block's exponent at 0
    x[3, 7] = value
    q, _, back = _roundtrip(x)
    assert back[3, 7].item() == want
    code = (int(q[3, 3]) >> 4) & 0xF  # element 7 = high nibble of byte 3
    assert GRID[code & 7] == abs(want) and bool(code & 8) == (value < 0)


def test_zero_block_and_packing():
    x = torch.zeros(64, 256)
    x[0, 32:64] = torch.arange(32) % 7 - 3.0
    q, s, back = _roundtrip(x)
    idx = ref.mxfp4_scale_index(64, 256)
    assert int(s[idx[0, 0]]) == 127 and int(s[idx[5, 3]]) == 127
    assert torch.equal(back, x)
    assert sorted(idx.reshape(-1).tolist()) == list(range(64 * 8))
    # bf16 input is widened, not re-rounded
    qb, sb = ops.quantize_mxfp4(x.bfloat16())
    assert torch.equal(qb, q) and torch.equal(sb, s)


def test_cpu_gemm_and_head_follow_the_decode():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(256, 256, generator=g), torch.randn(256, 256,
                                                           generator=g)
    (aq, sa), (bq, sb) = ops.quantize_mxfp4(a), ops.quantize_mxfp4(b)
    want = (ref.mxfp4_decode_cpu(aq, sa, 256)
            @ ref.mxfp4_decode_cpu(bq, sb, 256).t())
    assert torch.equal(ops.gemm_mxfp4_nt(aq, sa, bq, sb, out_fp32=True), want)
    b2, w3 = torch.randn(256, generator=g), torch.randn(256, generator=g)
    y = ops.gemm_mxfp4_relu_dot(aq, sa, bq, sb, b2, w3,
                                n_dev=torch.tensor([100]))
    torch.testing.assert_close(y[:100], (torch.relu(want + b2) @ w3)[:100])
    assert (y[100:] == 0).all()
    with pytest.raises(RuntimeError):
        ops.quantize_mxfp4(torch.zeros(32, 256))


# ---- the inputs of tests/test_mx4_edges_gpu.py, checked without a kernel ----

def _tile(x, t, per=256):
    return x[:, per * t:per * (t + 1)]


def _every_wave_tile_differs(d):
    """a difference somewhere in every 64 x 64 tile (one wave's share) of d"""
    R, C = d.shape
    return (d.reshape(R // 64, 64, C // 64, 64) != 0).any(axis=(1, 3)).all()


def _scale_swaps(va, ea, vb, eb, t, u):
    """tile t's products with tile u's scales on A, on B and on both, minus
    the true tile-t contribution to C"""
    def part(ta, tb):
        a = _tile(va, t) * np.repeat(np.exp2(_tile(ea, ta, 8)), 32, axis=1)
        b = _tile(vb, t) * np.repeat(np.exp2(_tile(eb, tb, 8)), 32, axis=1)
        return a @ b.T
    true = part(t, t)
    return [part(u, t) - true, part(t, u) - true, part(u, u) - true]


@pytest.mark.parametrize("K", list(mx4_data.KLOOP_PATHS))
def test_kloop_inputs_are_exact_and_see_a_wrong_k_tile(K):
    """What the exact GPU tests of the K-loop rest on.  The fp32 matmul
    equals the fp64 one, and C changes — somewhere in every wave's 64 x 64
    share — when one K-tile is dropped, counted twice, or multiplied with
    another tile's scales.  The one thing these inputs cannot see: their
    scale pattern repeats every three tiles, so scales taken from tile
    t +- 3 are the right ones; the ``free`` E8M0 inputs cover that."""
    case = mx4_data.kloop_case(K)
    a, b, c = case["a"], case["b"], case["c"]
    assert case["bound"] <= 117_323 and (a * 4 == (a * 4).round()).all()
    assert torch.equal((a @ b.t()).double(), c)
    assert torch.equal(ops.gemm_mxfp4_nt(*ops.quantize_mxfp4(a),
                                         *ops.quantize_mxfp4(b),
                                         out_fp32=True).double(), c)
    (va, ea), (vb, eb) = (
        [t.double().numpy() for t in mx4_data.grid_parts(512, seed, sp, K)]
        for seed, sp in ((1, (1, 1)), (2, (2, 1))))
    nt = K // 256
    for t in range(nt):
        # dropping tile t subtracts this, counting it twice adds it
        part = _tile(a, t).double().numpy() @ _tile(b, t).double().numpy().T
        assert _every_wave_tile_differs(part), t
        for u in range(nt):
            if u == t:
                continue
            if (t - u) % 3 == 0:
                assert np.array_equal(_tile(ea, t, 8), _tile(ea, u, 8))
                assert np.array_equal(_tile(eb, t, 8), _tile(eb, u, 8))
                continue
            for d in _scale_swaps(va, ea, vb, eb, t, u):
                assert _every_wave_tile_differs(d), (t, u)


@pytest.mark.parametrize("K, variant", [
    (256, "cancel"), (256, "spread"), (768, "cancel"), (768, "spread"),
    (1280, "free"), (1792, "free")])
def test_e8m0_inputs(K, variant):
    """The packed operands decode (oracle, fp64) to codes x 2^e; ``cancel``
    reaches scale bytes 0 and 254 on both operands; ``spread``
    outputs cover 2^+-80; exactness is asserted where the case is built.
    ``free`` sees any tile's products under any other tile's scales, on
    either operand or both."""
    case = mx4_data.e8m0_case(K, variant)
    for codes, exps, (q, s) in ((case["ca"], case["ea"], case["aq"]),
                                (case["cb"], case["eb"], case["bq"])):
        want = mx4_data.decode64(codes, exps)
        got = ref.mxfp4_decode_cpu(q, s, K, dtype=np.float64).numpy()
        assert np.array_equal(got, want)
        assert set(np.unique(codes)) == set(range(16))
        if variant == "cancel":
            assert s.min() == 0 and s.max() == 254
    a64 = torch.from_numpy(mx4_data.decode64(case["ca"], case["ea"]))
    b64 = torch.from_numpy(mx4_data.decode64(case["cb"], case["eb"]))
    assert torch.equal(a64 @ b64.t(), case["c"])
    if variant == "cancel":
        assert (case["ea"][:, :2] == [-127, 127]).all()
        assert (case["eb"][:, :2] == [127, -127]).all()
        # 6 * 2^127 is there and is beyond fp32
        assert np.abs(mx4_data.decode64(case["ca"], case["ea"])).max() \
            == 6 * 2.0 ** 127 > float(np.finfo(np.float32).max)
    if variant == "spread":
        mag = case["c"].abs()
        assert mag.max() > 2.0 ** 80 and mag[mag > 0].min() < 2.0 ** -80
    if variant == "free":
        va, vb = (mx4_data.code_values(case[k]) for k in ("ca", "cb"))
        ea, eb = case["ea"].astype(float), case["eb"].astype(float)
        nt = K // 256
        for t in range(nt):
            for u in range(nt):
                if u != t:
                    for d in _scale_swaps(va, ea, vb, eb, t, u):
                        assert _every_wave_tile_differs(d), (t, u)


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantiser_edges_oracle(dtype, K):
    """The oracle at the amaxes the device quantiser is compared on: the
    lower clamp (subnormals and exponent field 1 give byte 0), 6 * 2^k
    against its successor, and the largest binade (byte 253)."""
    x, where = mx4_data.edge_input(dtype, K)
    q, s = ops.quantize_mxfp4(x)
    idx = ref.mxfp4_scale_index(64, K)
    back = ref.mxfp4_decode_cpu(q, s, K, dtype=np.float64)
    for label, row, blk, pos, byte in where:
        assert int(s[idx[row, blk]]) == byte, (label, row, blk)
        v = x[row, 32 * blk + pos].double().item()
        got = back[row, 32 * blk + pos].item()
        if label == "min subnormal":
            want = 0.0          # 2^-149 (2^-133) / 2^-127 rounds to code 0
        elif label == "finfo.max":
            want = np.sign(v) * 2.0 ** 128  # 3.99.. * 2^126 rounds to 4
        elif label.startswith("above"):
            k = int(label.split("^")[1])
            want = np.sign(v) * 3 * 2.0 ** (k + 1)  # the same 6 * 2^k
        else:
            want = v            # on the grid of its own exponent
        assert got == want, (label, got, want)
        assert np.signbit(got) == np.signbit(v) or label == "min subnormal"
    labels = {w[0] for w in where}
    assert {"min subnormal", "subnormal 1.5*2^-127", "exponent field 1",
            "finfo.max"} <= labels and len(labels) == 12


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nonfinite_blocks_oracle(dtype, K):
    """The CPU twin of test_quantiser_nonfinite_blocks: scale byte 127, inf
    saturates to +-6, a NaN element gets ``E2M1_NAN_CODE`` with its own
    sign, and the finite neighbours get the codes they get at e = 0."""
    x, twin, where = mx4_data.nonfinite_input(dtype, K)
    q, s = ops.quantize_mxfp4(x)
    tq, ts = ops.quantize_mxfp4(twin)
    idx = ref.mxfp4_scale_index(64, K)
    for kind, row, blk, pos in where:
        assert int(s[idx[row, blk]]) == 127 == int(ts[idx[row, blk]])
        want = ((8 if kind[0] == "-" else 0)
                | (7 if "inf" in kind else ref.E2M1_NAN_CODE))
        assert mx4_data.nibble(q, row, 32 * blk + pos) == want, kind
    finite = torch.isfinite(x.float())
    assert torch.equal(s, ts)
    assert torch.equal(mx4_data.unpack(q)[finite],
                       mx4_data.unpack(tq)[finite])
    assert {k for k, *_ in where} == set(mx4_data.NONFINITE_BITS)


@pytest.mark.parametrize("out_fp32", [True, False])
@pytest.mark.parametrize("epilogue", ["plain", "relu", "bias_relu"])
def test_cpu_gemm_epilogues_exact(epilogue, out_fp32):
    """The oracle the GPU epilogue test compares with equals the fp64
    result, rounded once, on the same 256 x 256 x 768 inputs."""
    case = mx4_data.kloop_case(768)
    aq, sa = ops.quantize_mxfp4(case["a"][:256])
    bq, sb = ops.quantize_mxfp4(case["b"][:256])
    bias = case["b2"][:256] if epilogue == "bias_relu" else None
    pre = case["c"][:256, :256] + (0 if bias is None else bias.double())
    assert (pre < 0).any() and (pre > 0).any()
    want = (torch.relu(pre) if epilogue != "plain" else pre).float()
    got = ops.gemm_mxfp4_nt(aq, sa, bq, sb, bias, epilogue != "plain",
                            out_fp32)
    assert torch.equal(got, want if out_fp32 else want.bfloat16())


def test_expand1d_relu_of_a_negative_zero_is_plus_zero():
    """Without a bias 0 * w is -0 for a negative w.  The device's fmaxf
    makes it +0 (tests/test_mx4_edges_gpu.py found the CPU path keeping the
    sign, which put code 8 where the kernel writes 0)."""
    x = torch.tensor([0.0, 1.0, -1.0, 0.5] * 16)
    w = torch.tensor([-2.0, 3.0, 0.0, -0.5] * 64).bfloat16()
    q, s = ops.expand1d_mxfp4(x, w, None)
    h = x.double()[:, None] * w.double()[None, :]
    assert (torch.signbit(h) & (h == 0)).any()
    h = torch.where(h > 0, h, torch.zeros_like(h)).float()
    wq, ws = ref.quantize_mxfp4_cpu(h)
    assert torch.equal(q, wq) and torch.equal(s, ws)
    assert not (mx4_data.unpack(q) == 8).any()


def test_model_name_and_flags(monkeypatch):
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor
    from bodywork_mlops_demo_amd.pipeline.loop import resolve_model

    assert resolve_model("mlp-fp4") == ("mlp", {"BODYWORK_MLP_FP4": "1"})
    assert not GPUMLPRegressor(hidden=256).fp4_scoring
    monkeypatch.setenv("BODYWORK_MLP_FP4", "1")
    m_env = GPUMLPRegressor(hidden=256)
    assert m_env.fp4_scoring
    assert GPUMLPRegressor.from_sklearn(m_env.to_sklearn()).fp4_scoring
    monkeypatch.delenv("BODYWORK_MLP_FP4")
    m = GPUMLPRegressor(hidden=256, fp4_scoring=True)
    plain = GPUMLPRegressor(hidden=256)
    X = torch.rand(256) * 100
    # on the CPU predict takes the normal path, as with the fp8 flag
    assert torch.equal(m.predict(X), plain.predict(X))
    assert m._w2_q4 is None
