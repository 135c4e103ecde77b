"""GPU tests of the pack kernels behind the three width-generic fused kernels (msmp_pack_wide_msg_f32, msmp_pack_wide_tail_f32,
msmp_pack_lem_wide_f32): the blob is packed on the GPU, copied to the host and decoded with the layouts documented above the three
*Layout structs (wide_message_kernel.hip, wide_node_tail_kernel.hip, lem_wide_kernel.hip), restated here in numpy.

Every comparison is EXACT: the scale is a power of two (w * 2^s is the same float32 on both sides), numpy's float32 -> float16 cast rounds
to nearest even like (_Float16), and w - float32(hi) is one float32 subtraction on both sides.  The weights are uniform in +-0.3 with one
planted entry of larger magnitude per scale group, so the exponent s = 5 - e, frexp(max) = (m, e), is known from the inputs.

Widths 24 (one 32-channel slice, padding inside its k-steps) and 40 (two slices, the last one padded).  The LEM's `wxh` input-slot region
is a different layout and is not decoded here."""
import numpy as np
import pytest
import torch

from helpers import mp       # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

WIDTHS = [24, 40]
LANE, J = np.meshgrid(np.arange(64), np.arange(8), indexing='ij')       # [lane 64][j 8] of one fragment
C, HH = LANE & 31, LANE >> 5


def k_natural(ks):
    """split_k_natural (mfma_tiles.h) of every (lane, j) of k-step ks"""
    return 16 * ks + 8 * HH + J


def k_acc(ks):
    """split_k_acc within the 32-wide chunk ks // 2: the order in which accumulator registers become a B operand"""
    return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (J >> 2) + 4 * HH + (J & 3)


def weights(rng, shape, peak):
    """uniform in +-0.3 (no exact zeros), one entry planted at `peak`"""
    w = rng.uniform(0.01, 0.3, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    w = w.astype(np.float32)
    w.flat[int(rng.integers(w.size))] = peak
    return w


def shift_of(*arrays):
    """s with max |.| 2^s in [16, 32)"""
    mx = max(float(np.abs(a).max()) for a in arrays)
    e = int(np.frexp(np.float32(mx))[1])
    assert 16.0 <= mx * 2.0 ** (5 - e) < 32.0
    return 5 - e


def padded(m, rows, cols):
    out = np.zeros((rows, cols), dtype=np.float32)
    out[:m.shape[0], :m.shape[1]] = m
    return out


def split(x):
    """float32 [...] -> (hi, lo) float16: the 2-way split of the pack kernels"""
    x = x.astype(np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def fragments(blob, offset, n_frags):
    """the float16 region of n_frags (hi, lo) fragment pairs at float offset `offset` -> (hi, lo) as [n_frags, 64, 8]"""
    halfs = blob[offset:offset + 512 * n_frags].view(np.float16).reshape(n_frags, 2, 64, 8)
    return halfs[:, 0], halfs[:, 1]


def expected_fragments(mat, kt, n_ks, k_of):
    """[T kt][k-step n_ks][lane][j] of the zero-padded, scaled matrix `mat`: row 32 T + c, column k_of(ks)"""
    out = np.empty((kt, n_ks, 64, 8), dtype=np.float32)
    for T in range(kt):
        for ks in range(n_ks):
            out[T, ks] = mat[32 * T + C, k_of(ks)]
    return out.reshape(kt * n_ks, 64, 8)


def pack(mp, fn, tensors, ints, n_floats):
    from msmp_pde_amd._lib import ptr, current_stream
    dev = [torch.tensor(t, device='cuda') for t in tensors]
    blob = torch.full((n_floats,), float('nan'), dtype=torch.float32, device='cuda')       # every float of the blob must be written
    assert fn(*[ptr(t) for t in dev], *ints, ptr(blob), current_stream()) == 0
    torch.cuda.synchronize()
    return blob.cpu().numpy()


def check_scales(blob, shifts, extra=(0, 0)):
    want = np.zeros(8, dtype=np.float32)
    for i, s in enumerate(shifts):
        want[i] = 2.0 ** s
        want[4 + i] = 2.0 ** (-s - extra[i])
    assert np.array_equal(blob[:8], want)


def check_split(got, want):
    hi, lo = split(want)
    assert np.array_equal(got[0], hi)
    assert np.array_equal(got[1], lo)


@pytest.mark.parametrize('W', WIDTHS)
def test_message_blob(mp, W):
    L = mp.lib()
    kt = (W + 31) // 32
    Wp = 32 * kt
    rng = np.random.default_rng(10 + W)
    w2, b2 = weights(rng, (W, W), 0.75), weights(rng, (W,), 0.3)
    s = shift_of(w2, b2)
    assert s == 5
    n_floats = L.msmp_packed_wide_msg_floats(W)
    assert n_floats == 8 + Wp + 1024 * kt * kt
    blob = pack(mp, L.msmp_pack_wide_msg_f32, (w2, b2), (W,), n_floats)
    check_scales(blob, [s])
    sc = np.float32(2.0 ** s)
    assert np.array_equal(blob[8:8 + Wp], padded(b2[None] * sc, 1, Wp)[0])
    got = fragments(blob, 8 + Wp, kt * 2 * kt)
    check_split(got, expected_fragments(padded(w2 * sc, Wp, Wp), kt, 2 * kt, k_natural))
    # rows and columns >= W are exact zeros in both planes
    for plane in got:
        p = plane.reshape(kt, 2 * kt, 64, 8)
        for T in range(kt):
            for ks in range(2 * kt):
                dead = (32 * T + C >= W) | (k_natural(ks) >= W)
                assert not p[T, ks][dead].any()


@pytest.mark.parametrize('nv', [0, 3])
@pytest.mark.parametrize('W', WIDTHS)
def test_tail_blob(mp, W, nv):
    L = mp.lib()
    kt = (W + 31) // 32
    Wp, k1s = 32 * kt, 4 * kt + 1
    rng = np.random.default_rng(20 + W + nv)
    w3, b3 = weights(rng, (W, 2 * W + nv), 0.3), weights(rng, (W,), -0.75)      # the largest entry of the first group is in the BIAS
    w4, b4 = weights(rng, (W, W), -1.5), weights(rng, (W,), 0.3)
    s3, s4 = shift_of(w3, b3), shift_of(w4, b4)
    assert (s3, s4) == (5, 4)
    n_floats = L.msmp_packed_wide_tail_floats(W, nv)
    o_b3, o_b4, o_w3 = 8, 8 + Wp, 8 + 2 * Wp
    o_w4 = o_w3 + 512 * kt * k1s
    assert n_floats == o_w4 + 1024 * kt * kt
    blob = pack(mp, L.msmp_pack_wide_tail_f32, (w3, b3, w4, b4), (W, nv), n_floats)
    check_scales(blob, [s3, s4], extra=(8, 0))           # the node rows of GEMM 1 carry 2^8
    sc3, sc4 = np.float32(2.0 ** s3), np.float32(2.0 ** s4)
    assert np.array_equal(blob[o_b3:o_b3 + Wp], padded(b3[None] * np.float32(2.0 ** (s3 + 8)), 1, Wp)[0])
    assert np.array_equal(blob[o_b4:o_b4 + Wp], padded(b4[None] * sc4, 1, Wp)[0])
    # w3, natural order over [h columns: k-steps 0 .. 2 KT - 1 | agg columns: 2 KT .. 4 KT - 1 | the variables: one k-step, k = j on hh = 0]
    m3 = np.zeros((Wp, 2 * Wp + 16), dtype=np.float32)
    m3[:W, :W] = w3[:, :W] * sc3
    m3[:W, Wp:Wp + W] = w3[:, W:2 * W] * sc3
    m3[:W, 2 * Wp:2 * Wp + nv] = w3[:, 2 * W:] * sc3
    got3 = fragments(blob, o_w3, kt * k1s)
    check_split(got3, expected_fragments(m3, kt, k1s, k_natural))
    for plane in got3:
        p = plane.reshape(kt, k1s, 64, 8)
        for T in range(kt):
            assert not p[T, 4 * kt][HH == 1].any()                    # the hh = 1 half of the variables k-step
            assert not p[T, 4 * kt][J >= nv].any()                    # its columns j >= nv
            for ks in range(4 * kt):
                dead = (32 * T + C >= W) | (k_natural(ks % (2 * kt)) >= W)
                assert not p[T, ks][dead].any()
    live = (C < W) & (HH == 0) & (J < nv)                              # (slice 0's rows of the variables k-step)
    assert got3[0].reshape(kt, k1s, 64, 8)[0, 4 * kt][live].all()
    # w4, acc order
    got4 = fragments(blob, o_w4, kt * 2 * kt)
    check_split(got4, expected_fragments(padded(w4 * sc4, Wp, Wp), kt, 2 * kt, k_acc))
    for plane in got4:
        p = plane.reshape(kt, 2 * kt, 64, 8)
        for T in range(kt):
            for ks in range(2 * kt):
                assert not p[T, ks][(32 * T + C >= W) | (k_acc(ks) >= W)].any()


@pytest.mark.parametrize('W', WIDTHS)
def test_lem_rec_blob(mp, W):
    L = mp.lib()
    ninp = 3
    kt = (W + 31) // 32
    Wp, kin = 32 * kt, W + ninp
    rng = np.random.default_rng(30 + W)
    w, b = weights(rng, (3 * W, kin), 1.5), weights(rng, (3 * W,), 0.3)
    wz, bz = weights(rng, (W, kin), 0.3), weights(rng, (W,), 0.75)            # the largest entry of the second group is in the BIAS
    sw, sz = shift_of(w, b), shift_of(wz, bz)
    assert (sw, sz) == (4, 5)
    n_floats = L.msmp_packed_lem_wide_floats(ninp, W)
    assert n_floats == 8 + 4096 * kt * kt + 2048 * kt
    blob = pack(mp, L.msmp_pack_lem_wide_f32, (w, wz, b, bz), (ninp, W), n_floats)
    check_scales(blob, [sw, sz])
    # rec: [gate: g2, g3, g1, lin][T][k-step][plane][lane][8], acc order; g2, g3, g1 are rows W.., 2 W.., 0.. of `weights` (scale group 0),
    # lin is weights_lin_z (scale group 1); the recurrent columns are 0 .. W - 1 of each row
    gates = [w[W:2 * W, :W] * np.float32(2.0 ** sw), w[2 * W:, :W] * np.float32(2.0 ** sw), w[:W, :W] * np.float32(2.0 ** sw),
             wz[:, :W] * np.float32(2.0 ** sz)]
    got = fragments(blob, 8, 4 * kt * 2 * kt)
    want = np.concatenate([expected_fragments(padded(g, Wp, Wp), kt, 2 * kt, k_acc) for g in gates])
    check_split(got, want)
    for plane in got:
        p = plane.reshape(4, kt, 2 * kt, 64, 8)
        for T in range(kt):
            for ks in range(2 * kt):
                dead = (32 * T + C >= W) | (k_acc(ks) >= W)
                assert not p[:, T, ks][:, dead].any()
