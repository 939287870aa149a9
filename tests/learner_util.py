"""Shared inputs and references of the A2C learner tests (test infra): seeded minibatches, SB3's
A2C.train loss restated with torch modules (SB3 is not installed), and a float64 numpy
restatement of clip_grad_norm_ + RMSpropTFLike."""
import numpy as np
import torch

from policy_util import make_tensors, obs_rows

NETS = {"n32": [[32, 5], [32, 1]], "n64x32": [[64, 32, 8], [32, 64, 1]], "n96_3x32": [[96, 2], [32, 32, 32, 1]],
        "a2c": [[256, 256, 5], [256, 256, 1]], "w512": [[512, 5], [512, 1]]}
# Hyper-parameter sets away from the loop's (7e-4, 0.01, 0.5, 0.5, 0.99, 1e-5): the constructor's defaults (SB3's: no
# entropy bonus), no value loss, and every one moved at once.
HYPER_SETS = {
    "defaults": {},
    "vf0": dict(learning_rate=7e-4, ent_coef=0.01, vf_coef=0.0),
    "moved": dict(learning_rate=1e-2, ent_coef=0.0, vf_coef=0.25, max_grad_norm=0.1, alpha=0.9, rms_prop_eps=1e-8),
}
# D -> (G, R) of policy_geometries' e52 / e72; 107: the golden rows; 57, 87, 127, 347: test_gpu_learner's GEO
GEOMETRY = {52: (8, 4), 72: (10, 5), 107: None, 57: (9, 3), 87: (12, 7), 127: (12, 5), 347: (24, 6)}


def scale_pi_head(tensors, scale):
    """`tensors` with the pi head's weight matrix (not its bias) multiplied by `scale` in f32: the
    logit gaps grow by that factor and the softmax saturates.  The inputs are left as they are."""
    out = [[(w.copy(), b.copy()) for w, b in tw] for tw in tensors]
    w, b = out[0][-1]
    out[0][-1] = ((w * np.float32(scale)).astype(np.float32), b)
    return out


def minibatch(towers, D, rows, seed, head_scale=None):
    """(tensors, obs f32 [rows, D], actions i32, advantages f32, returns f32), seeded.  head_scale:
    scale_pi_head's factor (None: the tensors as drawn)."""
    rng = np.random.default_rng(1000 + seed)
    tensors = make_tensors(towers, D, seed, scale="var")
    if head_scale is not None:
        tensors = scale_pi_head(tensors, head_scale)
    obs = obs_rows(D, rows, seed=seed, geometry=GEOMETRY[D])
    actions = rng.integers(0, towers[0][-1], rows).astype(np.int32)
    adv = rng.standard_normal(rows).astype(np.float32)
    ret = (2.0 * rng.standard_normal(rows)).astype(np.float32)
    return tensors, obs, actions, adv, ret


def torch_a2c(tensors, activation, obs, actions, adv, ret, ent_coef, vf_coef, dtype):
    """A2C.train's loss (SB3 2.2.1, a2c.py: evaluate_actions, policy / value / entropy loss) and
    its autograd gradients in `dtype`: ([policy_loss, value_loss, entropy_loss, loss],
    [[(dW, db), ..], ..], scales) as float64 numbers / numpy arrays of `dtype`; scales: the mean
    absolute row term of each of the four scalars (mean |adv logp|, mean (ret - v)^2, mean |H| and
    their weighted sum), the size an error of a mean is measured against when the mean cancels."""
    act = torch.tanh if activation == "tanh" else torch.relu
    W = [[(torch.tensor(w, dtype=dtype, requires_grad=True), torch.tensor(b, dtype=dtype, requires_grad=True))
          for w, b in tw] for tw in tensors]
    x = torch.tensor(obs, dtype=dtype)
    heads = []
    for tw in W:
        h = x
        for i, (w, b) in enumerate(tw):
            h = torch.nn.functional.linear(h, w, b)
            h = act(h) if i < len(tw) - 1 else h
        heads.append(h)
    dist = torch.distributions.Categorical(logits=heads[0])
    log_prob = dist.log_prob(torch.tensor(actions, dtype=torch.long))
    policy_loss = -(torch.tensor(adv, dtype=dtype) * log_prob).mean()
    value_loss = torch.nn.functional.mse_loss(torch.tensor(ret, dtype=dtype), heads[1].flatten())
    entropy_loss = -torch.mean(dist.entropy())
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    loss.backward()
    s_pol = float((torch.tensor(adv, dtype=dtype) * log_prob).abs().mean().detach())
    s_val, s_ent = float(value_loss.detach()), float(dist.entropy().abs().mean().detach())
    return ([float(v.detach()) for v in (policy_loss, value_loss, entropy_loss, loss)],
            [[(w.grad.numpy(), b.grad.numpy()) for w, b in tw] for tw in W],
            [s_pol, s_val, s_ent, s_pol + ent_coef * s_ent + vf_coef * s_val])


def np_clip_rmsprop(params, sq, grads, lr, max_grad_norm, alpha, eps):
    """torch's clip_grad_norm_ and SB3's RMSpropTFLike (momentum 0, not centred) on flat float64
    arrays; returns (params, sq, norm, coef)."""
    g = np.asarray(grads, np.float64)
    norm = np.sqrt(np.sum(g * g))
    coef = min(1.0, max_grad_norm / (norm + 1e-6))
    g = g * coef
    sq = alpha * np.asarray(sq, np.float64) + (1.0 - alpha) * g * g
    return np.asarray(params, np.float64) - lr * g / np.sqrt(sq + eps), sq, norm, coef


def flat(tensors):
    """[[(w, b), ..], ..] -> one vector in the learner's order: tower, layer, weight then bias."""
    return np.concatenate([np.asarray(x).reshape(-1) for tw in tensors for wb in tw for x in wb])
