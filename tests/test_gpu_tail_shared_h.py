"""Gated node tail with the h rows staged and split ONCE for both heads (node_tail_split_kernel<true>).

The gate head and the main head consume the same fp16 fragments of h over chunks 0..3, each against its own W3 chunk and into its own
accumulator.  What that can break, and what equal-looking random weights could hide, is checked here against the float64 oracle:
graph ends on every wave boundary and beside it, heads whose h-columns differ as much as they can (one head's zeroed), the
rows around `out`, determinism, and the plain modes that share the chunk code.

Bar (the project's own, test_gpu_kernels.py::test_node_tail_vs_oracle): 5e-6 where every graph larger than one node has >= 30 nodes,
2e-4 otherwise.  Every size the issue lists is 1 or >= 31, so its split "along that line" leaves the looser call empty: both batches
are held to 5e-6 (`bar` below applies the rule to whatever sizes it is given)."""
import functools

import numpy as np
import pytest
import torch

from oracle import msmp_oracle as O

pytestmark = pytest.mark.gpu

H, TW, EPS = 128, 25, 1e-5
BATCHES = {
    'wave_ends': [1, 31, 32, 33, 64, 65, 96, 97, 100, 127, 128],
    'full_first_single_last': [128, 77, 1],
}
GUARD = 16      # NaN rows in front of and behind `out`


def bar(sizes):
    return 5e-6 if min(s for s in sizes if s > 1) >= 30 else 2e-4


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    msmp_pde_amd.lib()
    return msmp_pde_amd


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def rand_layer_sd(rng, nv, scale):
    k1, k3 = 2 * H + TW + 1 + nv, 2 * H + nv
    u = lambda *s, fan: (rng.uniform(-1, 1, s) / np.sqrt(fan) * scale).astype(np.float32)
    return {'message_net_1.0.weight': u(H, k1, fan=k1), 'message_net_1.0.bias': u(H, fan=k1),
            'message_net_2.0.weight': u(H, H, fan=H), 'message_net_2.0.bias': u(H, fan=H),
            'update_net_1.0.weight': u(H, k3, fan=k3), 'update_net_1.0.bias': u(H, fan=k3),
            'update_net_2.0.weight': u(H, H, fan=H), 'update_net_2.0.bias': u(H, fan=H)}


def pack(mp, sd, nv):
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    blob = torch.empty(L.msmp_packed_layer_floats(TW, nv), dtype=torch.float32, device='cuda')
    keys = ['message_net_1.0.weight', 'message_net_1.0.bias', 'message_net_2.0.weight', 'message_net_2.0.bias',
            'update_net_1.0.weight', 'update_net_1.0.bias', 'update_net_2.0.weight', 'update_net_2.0.bias']
    ts = [dev(sd[k]) for k in keys]
    check(L.msmp_pack_layer_f32(*[ptr(t) for t in ts], TW, nv, ptr(blob), current_stream()), 'pack')
    torch.cuda.synchronize()
    return blob


class Case:
    """Inputs of one (nv, batch): h, two DIFFERENT aggregates, two DIFFERENT random weight sets (index 0 = main head, 1 = gate head)."""

    def __init__(self, nv, name):
        self.nv, self.sizes = nv, BATCHES[name]
        rng = np.random.default_rng(4200 + 10 * nv + len(self.sizes))
        self.n = n = sum(self.sizes)
        self.batch = np.repeat(np.arange(len(self.sizes)), self.sizes)
        self.gptr = dev(np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32))
        self.h = rng.standard_normal((n, H)).astype(np.float32)
        self.var = rng.uniform(0, 1, (n, nv)).astype(np.float32)
        self.aggs = [rng.standard_normal((n, H)).astype(np.float32) for _ in range(2)]
        self.sds = [rand_layer_sd(rng, nv, scale=2.0) for _ in range(2)]
        self.dh, self.dvar, self.dagg = dev(self.h), dev(self.var), [dev(a) for a in self.aggs]

    def pre(self, sd, k, lin):
        p = O.layer_params({key: v.astype(np.float64) for key, v in sd.items()}, '')
        return O.instance_norm(O.node_update(p, self.h.astype(np.float64), self.aggs[k].astype(np.float64), self.var.astype(np.float64), lin), self.batch)

    def gated_ref(self, sds):
        tau = O.sigmoid(self.pre(sds[1], 1, True))
        return (1 - tau) * self.h.astype(np.float64) + tau * O.swish(self.pre(sds[0], 0, True))

    def run(self, mp, sds, gated=True, mode=1):
        """-> (out rows, guard rows in front, guard rows behind); `out` lies inside one NaN-filled allocation"""
        from msmp_pde_amd._lib import check, ptr, current_stream
        blobs = [pack(mp, sd, self.nv) for sd in sds]
        buf = torch.full((self.n + 2 * GUARD, H), float('nan'), device='cuda')
        out = buf[GUARD:GUARD + self.n]
        check(mp.lib().msmp_node_tail_f32(ptr(self.dh), ptr(self.dagg[0]), ptr(self.dagg[1]) if gated else None, ptr(self.dvar), ptr(self.gptr),
                                          self.n, len(self.sizes), max(self.sizes), self.nv, ptr(blobs[0]), ptr(blobs[1]) if gated else None,
                                          mode, EPS, ptr(out), current_stream()), 'node tail')
        torch.cuda.synchronize()
        return out.cpu(), buf[:GUARD].cpu(), buf[GUARD + self.n:].cpu()


@functools.lru_cache(maxsize=None)
def case(nv, name):
    return Case(nv, name)


@functools.lru_cache(maxsize=None)
def gated_reference(nv, name):
    c = case(nv, name)
    return c.gated_ref(c.sds)


def max_err(out, ref):
    return float(np.abs(out.double().numpy() - ref).max())


@pytest.mark.parametrize('name', list(BATCHES))
@pytest.mark.parametrize('nv', [1, 3, 8])
def test_gated_tail_vs_oracle(mp, nv, name):
    """Two different heads, two different aggregates, graph ends on and beside every wave boundary."""
    c = case(nv, name)
    out, _, _ = c.run(mp, c.sds)
    err = max_err(out, gated_reference(nv, name))
    print(f'gated tail nv={nv} {name}: max |hip - oracle| = {err:.3e} (bar {bar(c.sizes):.0e})')
    assert err < bar(c.sizes), err


@pytest.mark.parametrize('zeroed', [0, 1], ids=['main_h_columns_zero', 'gate_h_columns_zero'])
def test_heads_are_not_crossed(mp, zeroed):
    """One head's h-columns of W3 zeroed, the other's left random: a shared h phase that fed a chunk to the wrong head's weights or
    accumulator gives a result far from the oracle's."""
    c = case(3, 'wave_ends')
    sds = [dict(sd) for sd in c.sds]
    w = sds[zeroed]['update_net_1.0.weight'].copy()
    w[:, :H] = 0.0        # update_net_1 reads [h ; agg ; vars]
    sds[zeroed]['update_net_1.0.weight'] = w
    ref = c.gated_ref(sds)
    assert np.abs(ref - gated_reference(3, 'wave_ends')).max() > 1e-2      # (the zeroed head does change the result)
    out, _, _ = c.run(mp, sds)
    err = max_err(out, ref)
    print(f'heads not crossed, head {zeroed} without h: max |hip - oracle| = {err:.3e}')
    assert err < bar(c.sizes), err


@pytest.mark.parametrize('name', list(BATCHES))
def test_untouched_memory_and_determinism(mp, name):
    """The rows in front of and behind `out` keep their NaN, every row of `out` is written (finite), and a second call gives the same bits."""
    c = case(3, name)
    out, front, back = c.run(mp, c.sds)
    assert torch.isnan(front).all() and torch.isnan(back).all()
    assert torch.isfinite(out).all()
    out2, _, _ = c.run(mp, c.sds)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))


@pytest.mark.parametrize('mode,lin', [(1, True), (0, False)])
@pytest.mark.parametrize('nv', [1, 3, 8])
def test_plain_modes_vs_oracle(mp, nv, mode, lin):
    """agg_gate = None: the plain tail runs the same chunk code from chunk 0."""
    c = case(nv, 'wave_ends')
    out, front, back = c.run(mp, c.sds, gated=False, mode=mode)
    err = max_err(out, c.pre(c.sds[0], 0, lin))
    print(f'plain tail nv={nv} mode={mode}: max |hip - oracle| = {err:.3e}')
    assert torch.isnan(front).all() and torch.isnan(back).all()
    assert err < bar(c.sizes), err
