"""CPU test (no kernel launched): the C-ABI size queries of the layer forward / backward accept message_net_1 tails of up to four
32-column chunks (tw + 1 + nv <= 128: the 2-D classes at time_window 50) and refuse wider ones."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import msmp_pde_amd
    if not os.path.exists(msmp_pde_amd.LIB_PATH):       # hipcc cross-compiles gfx950 without a GPU
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return msmp_pde_amd.lib()


@pytest.mark.parametrize('tw,nv,stride', [(25, 2, 32), (50, 3, 64), (70, 3, 96), (100, 3, 128), (100, 8, 128), (127, 1, 160)])
def test_node_feature_stride(L, tw, nv, stride):
    assert L.msmp_node_feature_stride(tw, nv) == stride


def test_layer_backward_workspace_covers_four_tail_chunks(L):
    n, e = 800, 6400
    assert L.msmp_mp_layer_bwd_workspace_bytes(n, e, 50, 3, 1) > 0
    assert L.msmp_mp_layer_bwd_workspace_bytes(n, e, 100, 3, 1) > 0       # tw + 1 + nv = 104: four chunks
    assert L.msmp_mp_layer_bwd_workspace_bytes(n, e, 100, 8, 0) > 0          # tw + 1 + nv = 109
    assert L.msmp_mp_layer_bwd_workspace_bytes(n, e, 119, 8, 1) > 0          # 128: the bound
    assert L.msmp_mp_layer_bwd_workspace_bytes(n, e, 120, 8, 1) == 0         # 129: five chunks, refused
    assert L.msmp_mp_layer_bwd_workspace_bytes(n, e, 127, 1, 0) == 0         # stride 160, refused
