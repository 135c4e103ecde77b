"""Functional stand-in for the absent lem_cuda extension (its source is not in the reference tree).

Our own plain-torch statement of the published LEM cell, in the dtype of its arguments (the generator runs float64):

    X = [y, x_t];  g = X W^T + b, split into g1, g2, g3
    z <- (1 - dt s(g2)) z + dt s(g2) tanh(g3)
    y <- (1 - dt s(g1)) y + dt s(g1) tanh([z, x_t] Wz^T + bz)

`forward` returns the six tensors LEMFunction.forward unpacks; the first two are all_y_states and all_z_states, [T, N, nhid].
The cell arithmetic itself stays UNPINNED (nothing of the extension exists to compare with); what the reference's classes do
around the call is what the fixtures pin.  `backward` raises: no gradient of the reference's LEM is available."""
import torch


def forward(inputs, weights, weights_lin_z, bias, bias_lin_z, y0, z0, dt):
    nhid = weights_lin_z.shape[0]
    y, z = y0, z0
    ys, zs, xs, x2s, gates, lins = [], [], [], [], [], []
    for t in range(inputs.shape[0]):
        x = torch.cat((y, inputs[t]), 1)
        g = x @ weights.t() + bias
        dt_bar = dt * torch.sigmoid(g[:, :nhid])
        dt_z = dt * torch.sigmoid(g[:, nhid:2 * nhid])
        z = (1.0 - dt_z) * z + dt_z * torch.tanh(g[:, 2 * nhid:])
        x2 = torch.cat((z, inputs[t]), 1)
        lin = x2 @ weights_lin_z.t() + bias_lin_z
        y = (1.0 - dt_bar) * y + dt_bar * torch.tanh(lin)
        ys.append(y); zs.append(z); xs.append(x); x2s.append(x2); gates.append(g); lins.append(lin)
    return tuple(torch.stack(a) for a in (ys, zs, xs, x2s, gates, lins))


def backward(*a, **k):
    raise NotImplementedError('lem_cuda is absent from the reference tree: the stand-in has no backward')
