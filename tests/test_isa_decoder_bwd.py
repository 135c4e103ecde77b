"""Static check of the gfx950 code of the decoder backward kernels (no GPU: hipcc cross-compiles here, as in test_isa_gated_decoder.py).
Hard limits of every instantiated decoder_bwd_kernel: no scratch memory, and an LDS footprint that lets at least two workgroups share a
compute unit.  The vector-register count is printed (it goes into the profile note), not held to a number."""
import pytest

import isa

pytestmark = isa.needs_compiler()
LDS_PER_CU = 163840
# DecBwd<C, R, NETS, TW, K1, S1, K2, MODE>: 1-D tw 20 / 25 / 50 with the Euler update (MODE 1) and without (0), 2-D tw 25 / 50, gated 1-D / 2-D
GEOMETRIES = [(1, 128, 1, 20, 15, 4, 10, 1), (1, 128, 1, 25, 16, 3, 14, 1), (1, 128, 1, 50, 12, 2, 10, 1),
              (1, 128, 1, 20, 15, 4, 10, 0), (1, 128, 1, 25, 16, 3, 14, 0), (1, 128, 1, 50, 12, 2, 10, 0),
              (2, 128, 1, 25, 16, 3, 14, 1), (2, 128, 1, 50, 12, 2, 10, 1),
              (1, 82, 2, 25, 6, 2, 15, 2), (2, 82, 2, 25, 6, 2, 15, 2)]


def kernels():
    """{mangled name: kernel} of every decoder_bwd_kernel instantiation in the assembly"""
    return {k.name: k for k in isa.find('decoder_bwd_kernel.hip', r'_ZN4msmp\d+decoder_bwd_kernel')}


def test_every_geometry_is_instantiated():
    names = kernels()
    assert len(names) == len(GEOMETRIES), sorted(names)
    for g in GEOMETRIES:
        args = 'DecBwdI' + ''.join('Li%dE' % v for v in g)
        assert any(args in n for n in names), (g, sorted(names))


@pytest.mark.parametrize('geometry', GEOMETRIES)
def test_no_scratch_and_two_workgroups_per_compute_unit(geometry):
    args = 'DecBwdI' + ''.join('Li%dE' % v for v in geometry)
    r, = [r for n, r in kernels().items() if args in n]
    print(f'decoder_bwd_kernel<DecBwd<{", ".join(map(str, geometry))}>>: {r.vgpr} vector registers, {r.lds} bytes of LDS '
          f'({LDS_PER_CU // r.lds} workgroups per CU by LDS), scratch {r.scratch}')
    assert r.scratch == 0, r
    assert r.lds > 0 and LDS_PER_CU // r.lds >= 2, r
