"""CPU test (no kernel launched): the C-ABI size queries of the layer forward / backward accept message_net_1 tails of up to four
32-column chunks (tw + 1 + nv <= 128: the 2-D classes at time_window 50) and refuse wider ones."""
import pytest

from helpers import L        # noqa: F401  (a fixture)



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
