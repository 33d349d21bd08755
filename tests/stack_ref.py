"""The conv3p layer stack of include/conv3p.h (conv3p_stack_desc) on the CPU oracle, for any description.

    hidden layer l:  act_l = selu(Conv3p(points, act_{l-1}, W_l, strides[l], voxel)),   act_{-1} = input
    concat = [act_0 | act_1 | ...];   optional head:  head = selu(Conv3p(points, concat, W_head, strides[n_hidden], voxel))

The backward takes the gradient w.r.t. the head activation and / or the external gradient w.r.t. the concat
(`grad_concat`, added to each column block's gradient) and returns grad_input and every layer's grad_filter.  Built from
oracle.forward / oracle.backward (the pinned restatement of the reference op) and stack.selu_numpy / selu_grad_numpy.
The dtype of the arrays decides the precision: float32 arrays run the fp32 oracle, float64 arrays (points included) the
fp64 one, whose neighbour and tap decisions are then made in double, as the fp64 op makes them."""
import numpy as np

from oracle import oracle
from pointwise_amd import stack

VOX = 0.1
_MEMO = {}


def stack_reference(P, X, filters, strides, hidden, grad_head=None, grad_concat=None, voxel=VOX, nthreads=1, memo=None):
    """P (B, N, 3), X (B, N, in_channels), filters: n_hidden (+ 1 with a head) arrays (fz, fy, fx, Cin, Cout);
    strides: one (sx, sy, sz) per layer, the head's last.  grad_head (B, N, num_class): with a head; grad_concat
    (B, N, n_hidden * hidden) or None.  Returns (acts, grad_input, grad_filters): the hidden activations then the head
    activation, dL/dinput, one grad_filter per layer.  memo: a key under which the result is kept for the session."""
    if memo is not None and memo in _MEMO:
        return _MEMO[memo]
    kw = {"nthreads": nthreads} if nthreads > 1 else {}
    has_head = grad_head is not None
    nh = len(filters) - (1 if has_head else 0)
    assert len(strides) == len(filters) and nh >= 1
    assert grad_head is not None or grad_concat is not None, "the backward needs an external gradient"
    acts, x = [], X
    for l in range(nh):
        x = stack.selu_numpy(oracle.forward(P, x, filters[l], tuple(strides[l]), voxel, **kw))
        acts.append(x)
    dws = [None] * len(filters)
    ext = None
    if has_head:
        concat = np.concatenate(acts, axis=2)
        head = stack.selu_numpy(oracle.forward(P, concat, filters[nh], tuple(strides[nh]), voxel, **kw))
        acts.append(head)
        g = stack.selu_grad_numpy(head, grad_head)
        ext, dws[nh] = oracle.backward(g, P, concat, filters[nh], tuple(strides[nh]), voxel, **kw)
    if grad_concat is not None:
        ext = grad_concat if ext is None else ext + grad_concat
    carry = None
    for l in range(nh - 1, -1, -1):
        e = np.ascontiguousarray(ext[:, :, hidden * l:hidden * (l + 1)])
        g = stack.selu_grad_numpy(acts[l], e if carry is None else e + carry)
        carry, dws[l] = oracle.backward(g, P, acts[l - 1] if l > 0 else X, filters[l], tuple(strides[l]), voxel, **kw)
    out = (acts, carry, dws)
    if memo is not None:
        _MEMO[memo] = out
    return out
