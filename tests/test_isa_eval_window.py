"""Static check of the gfx950 code of eval_window_kernel (no GPU: hipcc cross-compiles here, as in test_isa_decoder_bwd.py).  Hard
limits: no scratch memory (the per-thread prediction registers of a chunk, pv[16], must stay registers), the LDS footprint the source
declares, and a vector-register count that lets four workgroups share a compute unit.  Nothing is asserted about instruction kinds."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'msmp-pde_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
LDS_BYTES = 64 * 65 * 4 + 2 * 256 * 8        # the [64, 65] float tile and the two [256] float64 partial tables
# The compiler reports 117 vector registers (hipcc -O3: sixteen prediction values, eight row segments in flight and their 64-bit
# addresses).  The bound asserted is the occupancy step above it: up to 128 registers a SIMD holds four waves, i.e. four resident
# 256-thread workgroups per compute unit.  A launch has batch * comps workgroups -- 16 or 32 at the evaluation batch sizes, on 256
# compute units -- so residency beyond that buys nothing; the next step down (96 registers, five waves) is not asserted.
VGPR_REPORTED, VGPR_LIMIT = 117, 128


@pytest.fixture(scope='module')
def resources(tmp_path_factory):
    d = tmp_path_factory.mktemp('isa_eval_window')
    s = d / 'eval_kernel.s'
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-S', '--cuda-device-only',
                    '-o', str(s), os.path.join(CSRC, 'eval_kernel.hip')], check=True, capture_output=True, cwd=str(d))
    isa = open(s).read()
    found = {}
    for k in re.finditer(r'^(_ZN4msmp\d+eval_window_kernel\w*):.*?\.end_amdhsa_kernel', isa, re.S | re.M):
        num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', k.group(0)).group(1))
        found[k.group(1)] = {'vgpr': num('next_free_vgpr'), 'scratch': num('private_segment_fixed_size'), 'lds': num('group_segment_fixed_size')}
    return found


def test_one_kernel_without_scratch_within_its_register_and_lds_budget(resources):
    assert len(resources) == 1, sorted(resources)
    (name, r), = resources.items()
    print(f'eval_window_kernel: {r["vgpr"]} vector registers (reported when this test was written: {VGPR_REPORTED}), {r["lds"]} bytes of LDS, '
          f'scratch {r["scratch"]}')
    assert r['scratch'] == 0, (name, r)
    assert r['lds'] == LDS_BYTES, (name, r)
    assert r['vgpr'] <= VGPR_LIMIT, (name, r)
