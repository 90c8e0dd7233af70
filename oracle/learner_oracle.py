"""numpy float64 restatement of the learner arithmetic. TEST INFRASTRUCTURE ONLY.

Written independently of hanabi_agents/rlax_dqn/learning.py (classic floor/ceil C51 projection instead of
the dense clip formulation) so that agreement between the two means something.
Sources: hanabi_agents/rlax_dqn/rlax_rainbow.py:172-200 (loss), hanabi_agents/rlax_dqn/noisy_mlp.py:61-91,176-185
(network), SURVEY.md Appendix B (rlax.categorical_double_q_learning, categorical_l2_project, optix.adam),
hanabi_agents/rainbow/rainbow_agent.py:252-404 (Dopamine's project_distribution, the worked example at :262-266).
Parity status: the reference learner cannot be imported here (jax/haiku/rlax absent) => "parity unpinned"
against a reference run; pinned by the Dopamine example and hand KATs in tests/test_learner.py.
The learner stages (c51_td_and_grad, dqn_td_and_grad, c51_backward, noisy_adam, per_priority) are additionally written
from hanabi_agents/rlax_dqn/rlax_dqn.py:160-205 (scalar double-Q), priority_buffer.py:48-52 (priorities) and
noisy_mlp.py (the merged weight w + w_mu + w_sigma * eps); they are pinned by central finite differences in
tests/test_learner.py and hold the GPU kernels in tests/test_learner_kernels_f64.py.
"""
import numpy as np


def softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=-1, keepdims=True)


def log_softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


def project_uniform(z_p, probs, vmin, vmax, k):
    """Classic C51 projection onto a uniform support of k atoms: mass of each source atom is split
    between its two neighbouring target atoms (floor/ceil form)."""
    delta = (vmax - vmin) / (k - 1)
    out = np.zeros(k)
    for zp, p in zip(z_p, probs):
        b = (min(max(zp, vmin), vmax) - vmin) / delta
        lo, hi = int(np.floor(b)), int(np.ceil(b))
        if lo == hi:
            out[lo] += p
        else:
            out[lo] += p * (hi - b)
            out[hi] += p * (b - lo)
    return out


def project_general(z_p, probs, z_q):
    """Projection onto an arbitrary sorted support (Dopamine project_distribution semantics)."""
    z_q = np.asarray(z_q, float)
    out = np.zeros(len(z_q))
    for zp, p in zip(z_p, probs):
        zp = min(max(zp, z_q[0]), z_q[-1])
        j = np.searchsorted(z_q, zp, side="right") - 1
        if j >= len(z_q) - 1:
            out[-1] += p
        else:
            w = (zp - z_q[j]) / (z_q[j + 1] - z_q[j])
            out[j] += p * (1 - w)
            out[j + 1] += p * w
    return out


def noisy_mlp_forward(x, layers):
    """layers: list of dicts w,b,w_mu,b_mu,w_sigma,b_sigma,eps_w,eps_b (noisy_mlp.py:61-91,176-185)."""
    out = np.asarray(x, float)
    for i, l in enumerate(layers):
        plain = out @ l["w"] + l["b"]
        noisy = out @ (l["w_mu"] + l["w_sigma"] * l["eps_w"]) + (l["b_mu"] + l["b_sigma"] * l["eps_b"])
        out = plain + noisy
        if i < len(layers) - 1:
            out = np.maximum(out, 0.0)
    return out


def c51_double_q_td(logits_tm1, a_tm1, r_t, discount, support, logits_t, logits_sel, terminal=None, bias_on=None,
                    bias_t=None, mask_terminal=True, parts=False):
    """Per-sample cross-entropy 'TD' of rlax_rainbow.py:172-185; logits [B, A, K].

    discount: scalar or per-sample [B] (gamma ** n of an n-step transition). terminal: zeroes the discount where set,
    unless mask_terminal is False (the reference's own update never masks: rlax_rainbow.py:178-180 is commented out).
    bias_on / bias_t: [A * K] output-layer biases added to the online (tm1 and selector) and the target logits.
    parts=True also returns the target distributions [B, K], the log-probabilities [B, K] of the taken action and the
    selected actions a* [B]."""
    b, a, k = logits_tm1.shape
    support = np.asarray(support, float)
    disc = np.broadcast_to(np.asarray(discount, float), (b,))
    bo = 0.0 if bias_on is None else np.asarray(bias_on, float).reshape(a, k)
    bt = 0.0 if bias_t is None else np.asarray(bias_t, float).reshape(a, k)
    td, tgt, logp, sel = np.zeros(b), np.zeros((b, k)), np.zeros((b, k)), np.zeros(b, np.int64)
    for i in range(b):
        q_sel = (softmax(logits_sel[i] + bo) * support[None]).mean(-1)   # mean, not sum (C-3)
        a_star = int(np.argmax(q_sel))                                   # the first maximum among ties
        p = softmax((logits_t[i] + bt)[a_star])
        g = disc[i] * (1.0 - terminal[i]) if (terminal is not None and mask_terminal) else disc[i]
        tgt[i] = project_uniform(r_t[i] + g * support, p, support[0], support[-1], k)
        logp[i] = log_softmax((logits_tm1[i] + bo)[a_tm1[i]])
        td[i] = -(tgt[i] * logp[i]).sum()
        sel[i] = a_star
    return (td, tgt, logp, sel) if parts else td


def is_weights(prios, beta, f32_inverse=False):
    """(1/P) ** beta / max. f32_inverse: 1/P cast to float32 first, as rlax_rainbow.py:188 does
    ((1. / prios).astype(jnp.float32)); the power and the normalisation stay in float64 here."""
    ip = 1.0 / np.asarray(prios, float)
    if f32_inverse:
        ip = ip.astype(np.float32).astype(float)
    w = ip ** beta
    return w / w.max()


def c51_td_and_grad(logits_tm1, logits_sel, logits_t, act, rew, term, disc, mask_terminal, support, prios, beta,
                    bias_on=None, bias_t=None):
    """td, IS weights and dLoss/dlogits of the taken action's K atoms for loss = mean(w * td) (rlax_rainbow.py:186-194).

    logits_* [B, A, K]; act [B]; rew, term, disc [B]; prios [B] sampling probabilities; beta scalar.
    The target is a constant (stop_gradient inside rlax.categorical_double_q_learning), so with
    td = -sum_k t_k log_softmax(l)_k:  d td / d l_k = softmax(l)_k * sum_j t_j - t_k, scaled by w / B.
    Returns (td [B], w [B], dl [B, K], a_star [B])."""
    logits_tm1 = np.asarray(logits_tm1, float)
    b = logits_tm1.shape[0]
    td, tgt, logp, sel = c51_double_q_td(logits_tm1, np.asarray(act), np.asarray(rew, float), disc, support,
                                         np.asarray(logits_t, float), np.asarray(logits_sel, float),
                                         np.asarray(term, float), bias_on, bias_t, bool(mask_terminal), parts=True)
    w = is_weights(prios, beta, f32_inverse=True)
    dl = (w / b)[:, None] * (np.exp(logp) * tgt.sum(-1, keepdims=True) - tgt)
    return td, w, dl, sel


def dqn_td_and_grad(q_tm1, q_sel, q_t, act, rew, term, disc, prios, beta, bias_on=None, bias_t=None):
    """Scalar double-Q learning of rlax_dqn.py:170-205: q_t zeroed where terminal, td = r + disc * q_t[argmax q_sel]
    - q_tm1[a]; loss = mean(w * l2_loss(td)) with l2_loss = td^2 / 2 (its clip_gradient(-1, 1) only clips the
    incoming cotangent 1.0: no effect). q_* [B, A]; bias_* [A]. Returns (td, w, dLoss/dq[b, a_tm1] [B], a_star)."""
    q_tm1, q_sel, q_t = (np.asarray(x, float) for x in (q_tm1, q_sel, q_t))
    b = q_tm1.shape[0]
    if bias_on is not None:
        q_tm1, q_sel = q_tm1 + np.asarray(bias_on, float), q_sel + np.asarray(bias_on, float)
    if bias_t is not None:
        q_t = q_t + np.asarray(bias_t, float)
    q_t = np.where(np.asarray(term)[:, None] != 0, 0.0, q_t)
    a_star = np.argmax(q_sel, axis=1)
    act = np.asarray(act)
    td = np.asarray(rew, float) + np.broadcast_to(np.asarray(disc, float), (b,)) * q_t[np.arange(b), a_star] - \
        q_tm1[np.arange(b), act]
    w = is_weights(prios, beta, f32_inverse=True)
    return td, w, -w * td / b, a_star


def c51_backward(dl, act, h, w2, k):
    """Backward of logits = h @ w2 + b2 for a gradient that lives in the taken action's K columns only.

    dl [B, K] (dLoss/dlogits[b, act[b] * K + k]); h [B, H] post-ReLU hidden activations; w2 [H, A * K].
    dH = relu'(h) * (dlogits @ w2^T) with relu'(0) = 0 (aten::threshold_backward: grad where h > 0);
    db1 = column sums of dH; dW2 = h^T @ dlogits; db2 = column sums of dlogits.
    Returns (dH [B, H], db1 [H], dW2 [H, A * K], db2 [A * K])."""
    dl, h, w2 = (np.asarray(x, float) for x in (dl, h, w2))
    b = dl.shape[0]
    dense = np.zeros((b, w2.shape[1]))
    for i in range(b):
        dense[i, act[i] * k:(act[i] + 1) * k] = dl[i]
    dh = np.where(h > 0, dense @ w2.T, 0.0)
    return dh, dh.sum(0), h.T @ dense, dense.sum(0)


def noisy_adam(w, w_mu, w_sigma, noise, g, moments, t, lr=1e-3, b1=0.9, b2=0.999, eps=3.125e-5, step_offset=0.0,
               shared=False):
    """One optix.adam step (adam_step) on the three parameters of a NoisyLinear weight, given the gradient g of the
    merged weight W = w + w_mu + w_sigma * noise (noisy_mlp.py): dW/dw = dW/dw_mu = 1, dW/dw_sigma = noise.

    moments: (m_w, v_w, m_mu, v_mu, m_sigma, v_sigma); shared=True: w_mu takes w's step and moments (m_mu, v_mu are
    ignored and returned unchanged) — equal gradients keep equal moments. t: completed steps; this step is
    t + step_offset. Returns (w, w_mu, w_sigma, moments, eff) with eff = w + w_mu + w_sigma * noise after the step."""
    m_w, v_w, m_mu, v_mu, m_sg, v_sg = (np.asarray(x, float) for x in moments)
    g, noise = np.asarray(g, float), np.asarray(noise, float)
    tt = t + step_offset
    w, m_w, v_w = adam_step(np.asarray(w, float), g, m_w, v_w, tt, lr, b1, b2, eps)
    if shared:
        w_mu = np.asarray(w_mu, float) - lr * (m_w / (1 - b1 ** tt)) / (np.sqrt(v_w / (1 - b2 ** tt)) + eps)
    else:
        w_mu, m_mu, v_mu = adam_step(np.asarray(w_mu, float), g, m_mu, v_mu, tt, lr, b1, b2, eps)
    w_sigma, m_sg, v_sg = adam_step(np.asarray(w_sigma, float), g * noise, m_sg, v_sg, tt, lr, b1, b2, eps)
    return w, w_mu, w_sigma, (m_w, v_w, m_mu, v_mu, m_sg, v_sg), w + w_mu + w_sigma * noise


def per_priority(td, alpha):
    """update_priorities of priority_buffer.py:48-52: (priorities + 1e-10) ** alpha with priorities = |td| (float32,
    rlax_rainbow.py:198). A float32 array plus / to the power of a Python float stays float32, so the sum and the
    exponent are float32 values; the power is taken in float64 and rounded once to float32 (the correctly rounded
    float32 result). Returns float32."""
    x = np.abs(np.asarray(td, np.float32)) + np.float32(1e-10)
    return (x.astype(float) ** float(np.float32(alpha))).astype(np.float32)


def adam_step(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=3.125e-5):
    """optix.adam: eps outside the square root; t counts from 1."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mhat, vhat = m / (1 - b1 ** t), v / (1 - b2 ** t)
    return p - lr * mhat / (np.sqrt(vhat) + eps), m, v
