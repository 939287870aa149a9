"""Shared inputs of the bf16 policy tests (test infra): bf16 rounding in numpy, the f64 reference
and torch's own bf16 modules as the accuracy yardstick, and the lattice generator of the
"exact" cases -- weights and obs for which every partial sum of every hidden pre-activation is
exactly representable in f32, so the kernel and the host twin must agree bit for bit whatever
order the hardware sums in.

The lattice.  A layer's operands lie on power-of-two grids: x on 2^-gx, W on 2^-gw, so every
term w x of a pre-activation is a multiple of 2^-g, g = gx + gw, and so is the bias.  If
sum |terms| + |bias| < 2^(20 - g), every partial sum in any order is an integer below 2^20 times
2^-g: 20 significant bits, 4 bits of headroom under f32's 24.  A ReLU activation rounded to bf16
stays on the grid 2^-g (rounding a multiple of 2^-g to fewer significant bits gives a multiple
of 2^-g) and below the bound, which makes it the next layer's x.  A tanh activation is not on
a grid, so tanh cases have one hidden layer (exact pre-activation, the same pe_tanhf, the same
rounding).  `lattice_check` asserts all of that from the tensors themselves.

Construction: obs are m 2^-6, 1 <= |m| <= 255 (8-bit significands); first-layer weights are
+-{1, 2, 3} 2^-6 on the k with (k + j) % P == 0, P about K / 8; deeper weights are +-1 on two k
per neuron, P = K / 2 (small enough for three ReLU layers on the grid of a code table);
biases are m 2^-6, |m| <= 3.  P <= N and P <= K, so a nonzero weight reaches every k -- the last
before the pad included -- and every neuron.
"""
import numpy as np
import torch

# (grid, plants, obstacles, range, channels), the obs forms fed to a policy; D = 5 C + 27 by its
# residue mod 16, the bf16 kernel's k step: 11, 13, 4, 8, 1 and 0 (c17: no padded k at all)
GEO = {
    "g20": dict(cfg=(20, 10, 12, 6, 16), obs=("codes",)),     # D = 107
    "g21": dict(cfg=(21, 8, 50, 2, 10), obs=("f32",)),        # D = 77
    "e52": dict(cfg=(8, 3, 3, 4, 5), obs=("codes",)),         # D = 52
    "e72": dict(cfg=(10, 4, 4, 5, 9), obs=("codes",)),        # D = 72
    "max417": dict(cfg=(12, 4, 6, 3, 78), obs=("f32",)),      # D = 417
    "c17": dict(cfg=(12, 4, 6, 7, 17), obs=("codes", "f32")),  # D = 112
}
# the exact cases: one hidden layer with tanh and relu, two towers, A2C's and DQN's widths with
# relu (DQN's 512-wide layers are 16 neuron tiles over 8 waves: a second pass)
EXACT_NETS = [
    ([[32, 5]], "tanh"),
    ([[32, 5]], "relu"),
    ([[32, 5], [32, 1]], "tanh"),
    ([[256, 256, 5], [256, 256, 1]], "relu"),
    ([[512, 512, 256, 5]], "relu"),
]
LATTICE_SEED = 4242


def obs_dim(name):
    return 5 * GEO[name]["cfg"][4] + 27


def exact_x_values(name, form):
    """Every value an obs entry of an exact case can take, rounded to bf16: the lattice of
    lattice_obs for f32 obs, the geometry's code table for codes."""
    if form == "f32":
        return np.arange(-255, 256, dtype=np.float32) / 64.0
    from plantos_amd.codes import code_table
    G, _, _, R, _ = GEO[name]["cfg"]
    return bf16_round(code_table(G, R))


def bf16_round(x):
    """float32 array rounded to bf16, to nearest even, as float32 (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def grid_log2(v):
    """The smallest g >= 0 with every value of v a multiple of 2^-g."""
    v = np.asarray(v, np.float64).ravel()
    for g in range(0, 64):
        s = v * 2.0 ** g
        if np.array_equal(s, np.rint(s)):
            return g
    raise AssertionError("values are on no grid down to 2^-63")


def lattice_obs(rows, D, seed):
    """f32 [rows, D]: m 2^-6 with 1 <= |m| <= 255."""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 256, (rows, D)) * rng.choice((-1, 1), (rows, D))
    return np.ascontiguousarray(m / 64.0, np.float32)


def lattice_tensors(towers, D, seed):
    """numpy f32 [(W, b), ..] per tower: lattice hidden layers (module docstring), heads N(0, 1) / 8."""
    rng = np.random.default_rng(seed)
    out = []
    for t in towers:
        K, tw = D, []
        for l, N in enumerate(t):
            if l == len(t) - 1:  # the head is f32 and defined bit for bit: any weights
                W = (rng.standard_normal((N, K)) / 8).astype(np.float32)
                b = (rng.standard_normal(N) / 8).astype(np.float32)
            else:
                P = min(N, K, max(8, -(-K // 8))) if l == 0 else min(N, K // 2)
                j, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
                mag = rng.integers(1, 4, (N, K)) / 64.0 if l == 0 else np.ones((N, K))
                W = np.where((k + j) % P == 0, mag * rng.choice((-1.0, 1.0), (N, K)), 0.0).astype(np.float32)
                b = (rng.integers(-3, 4, N) / 64.0).astype(np.float32)
            tw.append((W, b))
            K = N
        out.append(tw)
    return out


def lattice_check(towers, tensors, activation, x_values):
    """Asserts that (towers, tensors) are exact for obs rows drawn from `x_values` (every value an
    obs entry can take, already rounded to bf16): grids, bounds, bf16 operands, no subnormals, and
    nonzero weights on every k and every neuron of every hidden layer.  Returns [(tower, layer, g,
    bound, limit), ..]."""
    x_values = np.asarray(x_values, np.float32)
    assert np.array_equal(bf16_round(x_values), x_values)
    tiny = float(np.finfo(np.float32).tiny)
    assert all(abs(float(v)) >= tiny for v in x_values.ravel() if v != 0)
    rows = []
    for ti, (t, tw) in enumerate(zip(towers, tensors)):
        if activation == "tanh":
            assert len(t) == 2, "tanh activations are on no grid: one hidden layer only"
        g_in, a_max = grid_log2(x_values), float(np.abs(x_values).max())
        for l, (W, b) in enumerate(tw[:-1]):
            W64, b64 = W.astype(np.float64), b.astype(np.float64)
            assert np.array_equal(bf16_round(W), W), (ti, l)
            assert np.all((W == 0) | (np.abs(W64) >= tiny))
            assert (W != 0).any(axis=0).all() and (W != 0).any(axis=1).all() and (W[:, -1] != 0).any(), (ti, l)
            g = g_in + grid_log2(W)
            assert grid_log2(b) <= g, (ti, l)
            bound = float((np.abs(W64).sum(axis=1) * a_max + np.abs(b64)).max())
            limit = 2.0 ** (20 - g)
            assert bound < limit, (ti, l, g, bound, limit)
            rows.append((ti, l, g, bound, limit))
            g_in, a_max = g, max(bound, float(bf16_round(np.float32(bound))))  # |bf16(relu(z))| <= either
    return rows


def reference_heads(tensors, activation, obs):
    """[head of tower 0 [n, A], head of tower 1 [n, 1] ..] in float64 torch on the f32 weights."""
    act = torch.tanh if activation == "tanh" else torch.relu
    out = []
    for tw in tensors:
        x = torch.as_tensor(np.asarray(obs, np.float32)).double()
        for l, (W, b) in enumerate(tw):
            W, b = torch.as_tensor(np.asarray(W)).double(), torch.as_tensor(np.asarray(b)).double()
            x = x @ W.T + b
            if l < len(tw) - 1:
                x = act(x)
        out.append(x.numpy())
    return out


def torch_bf16_heads(tensors, activation, obs):
    """The yardstick: torch's own modules in torch.bfloat16 on the CPU -- weights, biases, inputs
    and activations all bf16 -- as float64 arrays like reference_heads'."""
    out = []
    for tw in tensors:
        mods = []
        for l, (W, b) in enumerate(tw):
            lin = torch.nn.Linear(W.shape[1], W.shape[0])
            with torch.no_grad():
                lin.weight.copy_(torch.as_tensor(np.asarray(W)))
                lin.bias.copy_(torch.as_tensor(np.asarray(b)))
            mods.append(lin)
            if l < len(tw) - 1:
                mods.append(torch.nn.Tanh() if activation == "tanh" else torch.nn.ReLU())
        net = torch.nn.Sequential(*mods).to(torch.bfloat16)
        with torch.no_grad():
            y = net(torch.as_tensor(np.asarray(obs, np.float32)).to(torch.bfloat16))
        out.append(y.double().numpy())
    return out


def worst_deviation(heads, ref):
    """max |head - reference| over every tower's head; heads: (logits [n, A], values [n] or None)."""
    logits, values = heads
    d = float(np.abs(np.asarray(logits, np.float64) - ref[0]).max())
    if values is not None:
        d = max(d, float(np.abs(np.asarray(values, np.float64) - ref[1][:, 0]).max()))
    return d


def np_tensors(tensors):
    """parse_state_dict's tensors (or numpy) as numpy f32 [(W, b), ..] per tower."""
    f = lambda x: x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()  # noqa: E731
    return [[(np.ascontiguousarray(f(W), np.float32), np.ascontiguousarray(f(b), np.float32)) for W, b in tw]
            for tw in tensors]
