"""Factorised per-UAV policy head for the CNN and the MLP actor-critic: one n_act-way softmax per UAV instead of the reference's one softmax over the
N_A = 5^nBS joint actions (main.py:143-156), which cannot be built beyond a handful of UAVs (1.5e11 logits at 16).  An extension beyond
the reference, like the search policies; DESIGN.md section 17.

  layout    A = n_act (5), B = n_heads = nBS.  Logits z [M, B*A]; head b = columns [b*A, (b+1)*A); p_b = softmax(z_b); the joint
            probability is the product over the heads.
  action    a = sum_b d_b * A^(B-1-b), UAV 0 the most significant digit: Decimal_to_Base_N (ue_mobility.py:310-336), the order every
            policy of this package uses (heuristics.coordinate_rule).
  draw      per head, the rule of agent.sample_actions: the first digit d with cumsum(p_b)[d] > u[row, b] * cumsum(p_b)[-1].
  loss      main.py:64-74 with the product policy, the reference's + 1e-5 once per head:
            logp = sum_b log(p_b[d_b] + 1e-5);  H = sum_b -sum_j p_bj log(p_bj + 1e-5);  a_loss = mean(-(beta * H + logp * td)).
            With B = 1 this is agent.a2c_losses term for term.

On the GPU the draw, the greedy choice and the loss gradient are libuavagent.so's (csrc/agent_factored.hip); everything else -- trunks,
head GEMMs, RMSProp, rollout, checkpoint -- is cnn_agent's (FactoredCnn*) or agent's (FactoredACNet / FactoredA2CRunner), unchanged.  The MLP's
first layer holds one table row per observation node: beyond 64 nodes (16 UAV + 200 UE = 216) it runs on the 256-node gather and table
gradient of csrc/agent_wide.hip.  FactoredA2CRunner.ppo_rollout runs PPO on the same update path: GAE(lambda)
advantages and several clipped-surrogate epochs per rollout on the kernels of csrc/agent_ppo.hip.
FactoredA2CRunner(mask_margin=m) takes the moves BS_move would not commit, and those ending within m cells of another UAV, out of the
policy's support: one masking pass (csrc/agent_mask.hip) in front of the draw and the losses.
"""
import torch

from .agent import ENTROPY_BETA, HIDDEN, A2CRunner, ACNet, _ppo_clipped, gae_reference      # noqa: F401 (gae_reference stays importable from here)
from .cnn_agent import CnnA2CRunner, CnnACNet, _logits_cuda, _trunks_cuda, _value_cuda

N_ACT = 5     # mobile_env.py:21


def joint_to_digits(actions, n_heads, n_act=N_ACT):
    """Joint actions int64 [...] -> digits int64 [..., n_heads], d_b = (a // n_act^(n_heads-1-b)) mod n_act (integer arithmetic: exact for
    every action below 2^63)."""
    a = torch.as_tensor(actions, dtype=torch.int64)
    out = []
    for _ in range(int(n_heads)):
        out.append(a % n_act)
        a = a // n_act
    return torch.stack(out[::-1], dim=-1)


def digits_to_joint(digits, n_act=N_ACT):
    """Digits [..., n_heads] -> joint actions int64 [...], Horner's rule in int64: exact up to n_act^n_heads - 1 <= 2^63 - 1 (5^27 - 1)."""
    d = torch.as_tensor(digits).to(torch.int64)
    a = torch.zeros(d.shape[:-1], dtype=torch.int64, device=d.device)
    for b in range(d.shape[-1]):
        a = a * n_act + d[..., b]
    return a


def _heads(head_prob):
    if head_prob.dim() != 3:
        raise ValueError("per-head probabilities must be [M, n_heads, n_act]")
    return head_prob


def sample_actions_factored(head_prob, uniforms, return_digits=False):
    """One joint action per row of head_prob [M, B, A] with the uniforms [M, B]: agent.sample_actions per head (cdf = cumsum(p_b); the
    first digit with cdf > u * cdf[-1], i.e. searchsorted(side='right'); clamped to A - 1), the digits composed by digits_to_joint."""
    p = _heads(head_prob)
    M, B, A = p.shape
    cdf = p.cumsum(dim=2)
    u = uniforms.reshape(M, B, 1).to(p.dtype) * cdf[:, :, -1:]
    d = torch.searchsorted(cdf, u, right=True).squeeze(2).clamp_(max=A - 1)
    a = digits_to_joint(d, A)
    return (a, d) if return_digits else a


def a2c_losses_factored(head_prob, v, actions, v_target, beta=ENTROPY_BETA):
    """(a_loss, c_loss) of main.py:64-74 for the product policy.  head_prob [M, B, A], v and v_target [M, 1], actions = JOINT actions [M]."""
    p = _heads(head_prob)
    M, B, A = p.shape
    d = joint_to_digits(actions.reshape(-1), B, A)                              # [M, B]
    td = v_target - v                                                           # :64
    c_loss = (td ** 2).mean()                                                   # :66
    log_prob = torch.log(p.gather(2, d.unsqueeze(2)).squeeze(2) + 1e-5).sum(dim=1, keepdim=True)   # :69, one + 1e-5 per head
    exp_v = log_prob * td.detach()                                              # :70
    entropy = -(p * torch.log(p + 1e-5)).sum(dim=(1, 2)).reshape(M, 1)          # :71-72, the entropy of a product = the sum over heads
    a_loss = (-(beta * entropy + exp_v)).mean()                                 # :73-74
    return a_loss, c_loss


def loss_grad_factored_reference(logits, v, v_target, actions, n_heads, n_act=N_ACT, beta=ENTROPY_BETA):
    """The closed-form gradient uavagent_a2c_loss_grad_factored implements, in PyTorch (dtype of logits).  With p = softmax(z_b), e = 1e-5:
        gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - [j == d_b] td / (p_{d_b} + e);   d a_loss / d z_j = p_j (gp_j - sum_i p_i gp_i) / M
    head by head (the heads are separate terms of the loss), d c_loss / d v = -2 td / M.
    -> (dlogits [M, B*A], dv [M], dbias [B*A] = column sums of dlogits, (a_loss, c_loss, sum(dv)))."""
    M, B, A = logits.shape[0], int(n_heads), int(n_act)
    z = logits.reshape(M, B, A)
    p = torch.softmax(z, dim=2)
    n_joint = A ** B
    d = joint_to_digits(actions.reshape(-1).clamp(0, n_joint - 1), B, A)        # the kernel's clamp: no action is used as an index
    td = (v_target.reshape(M) - v.reshape(M)).to(z.dtype)
    lp = torch.log(p + 1e-5)
    gp = beta * (lp + p / (p + 1e-5))
    hot = torch.zeros_like(p).scatter_(2, d.unsqueeze(2), 1.0)
    gp = gp - hot * (td.reshape(M, 1, 1) / (p + 1e-5))
    dot = (p * gp).sum(dim=2, keepdim=True)
    dz = (p * (gp - dot) / M).reshape(M, B * A)
    dv = -2.0 * td / M
    h = -(p * lp).sum(dim=(1, 2))
    logp = (lp * hot).sum(dim=(1, 2))
    a_loss = (-(beta * h + logp * td)).mean()
    return dz, dv, dz.sum(dim=0), (a_loss, (td ** 2).mean(), dv.sum())


# ---- move masking: a masked digit's logit counts as -inf -- p = 0, no entropy term, no gradient ------------------------
def allowed_from_idx(idx, n_heads, grid_n, bs_step, min_bs_dist, margin):
    """heuristics.move_mask in torch, from index rows: idx int64 [M, K >= n_heads] whose first n_heads entries are the UAV cells x * G + y
    (agent.obs_to_indices) -> bool [M, n_heads, 5] on idx's device.  A row with a negative cell (first_state="zeros") allows everything,
    as uavagent_mask_move_logits_f32 leaves it alone."""
    B, G, s, D, m = int(n_heads), int(grid_n), int(bs_step), int(min_bs_dist), int(margin)
    c = idx[:, :B]
    blank = (c < 0).any(dim=1)
    c = c.clamp(min=0)
    x, y = torch.div(c, G, rounding_mode="floor"), c % G
    xy = torch.stack([x, y], dim=-1)                                                        # [M, B, 2]
    ok = torch.stack([x + s < G, x - s > 1, y + s < G, y - s > 1], dim=-1)                  # [M, B, 4]
    eye = torch.eye(B, dtype=torch.bool, device=idx.device)
    d2 = ((xy[:, :, None, :] - xy[:, None, :, :]) ** 2).sum(-1)
    ok = ok & ~((d2 <= D * D) & ~eye).any(-1)[:, :, None]
    if m > 0 and B > 1:
        delta = torch.tensor(((1, 0), (-1, 0), (0, 1), (0, -1)), dtype=torch.int64, device=idx.device) * s
        dest = xy[:, :, None, :] + delta                                                    # [M, B, 4, 2]
        e2 = ((dest[:, :, :, None, :] - xy[:, None, None, :, :]) ** 2).sum(-1)             # [M, B, 4, B]
        ok = ok & ~((e2 <= m * m) & ~eye[:, None, :]).any(-1)
    allowed = torch.cat([ok, torch.ones_like(ok[:, :, :1])], dim=-1)
    return allowed | blank[:, None, None]


def mask_logits(logits, allowed):
    """logits [M, B * A] or [M, B, A] with the digits not ``allowed`` (bool [M, B, A]) at -inf, as [M, B, A]: the masked forms of every
    function of this module are the function itself on these logits (softmax gives p = 0 there: no entropy term, no gradient)."""
    M, B, A = allowed.shape
    return logits.reshape(M, B, A).masked_fill(~allowed, float("-inf"))


def masked_head_prob(logits, allowed):
    """Per-head probabilities [M, B, A] under the mask: softmax(mask_logits(logits, allowed)) over the digits."""
    return torch.softmax(mask_logits(logits, allowed), dim=2)


def loss_grad_factored_reference_masked(logits, allowed, v, v_target, actions, beta=ENTROPY_BETA):
    """loss_grad_factored_reference under the mask ``allowed`` bool [M, B, A]: dlogits is exactly 0 at the masked columns."""
    M, B, A = allowed.shape
    return loss_grad_factored_reference(mask_logits(logits, allowed).reshape(M, B * A), v, v_target, actions, B, A, beta)


def ppo_loss_grad_factored_reference_masked(logits, allowed, v, ret, adv, logp_old, actions, beta=ENTROPY_BETA, clip=0.2):
    """ppo_loss_grad_factored_reference under the mask ``allowed`` bool [M, B, A]."""
    M, B, A = allowed.shape
    return ppo_loss_grad_factored_reference(mask_logits(logits, allowed).reshape(M, B * A), v, ret, adv, logp_old, actions, B, A, beta, clip)


def check_mask_margin(margin):
    """-> None or the margin as an int >= 0; ValueError otherwise."""
    if margin is None:
        return None
    if isinstance(margin, bool) or int(margin) != margin or int(margin) < 0:
        raise ValueError("mask_margin must be None or an integer >= 0")
    return int(margin)


# ---- PPO: GAE(lambda) advantages and the clipped surrogate in place of the chosen-action term -----------------------
def logp_factored(head_prob, actions):
    """log pi(a | s) = sum_b log(p_b[d_b] + 1e-5) of the JOINT actions [M] under head_prob [M, B, A] (the kernel's clamp of the actions) -> [M]."""
    p = _heads(head_prob)
    M, B, A = p.shape
    d = joint_to_digits(actions.reshape(-1).clamp(0, A ** B - 1), B, A)
    return torch.log(p.gather(2, d.unsqueeze(2)).squeeze(2) + 1e-5).sum(dim=1)


def ppo_losses_factored(head_prob, v, actions, adv, ret, logp_old, beta=ENTROPY_BETA, clip=0.2):
    """(a_loss, c_loss) of PPO for the product policy, differentiable.  head_prob [M, B, A], v [M, 1], actions = JOINT actions [M]; adv, ret and
    logp_old [M] (or [M, 1]) are constants.  rho = exp(logp - logp_old); a row is clipped when (adv > 0 and rho > 1 + clip) or (adv < 0 and
    rho < 1 - clip); s = clipped ? clamp(rho, 1 - clip, 1 + clip) adv : rho adv;  a_loss = mean(-s - beta sum_b H_b), H_b as in
    a2c_losses_factored;  c_loss = mean((ret - v)^2)."""
    p = _heads(head_prob)
    M = p.shape[0]
    adv, ret, logp_old = (t.reshape(M).detach().to(p.dtype) for t in (adv, ret, logp_old))
    rho = torch.exp(logp_factored(p, actions) - logp_old)
    clipped = _ppo_clipped(rho.detach(), adv, clip)
    s = torch.where(clipped, rho.detach().clamp(1.0 - clip, 1.0 + clip), rho) * adv       # a clipped row is a constant of the parameters
    entropy = -(p * torch.log(p + 1e-5)).sum(dim=(1, 2))
    a_loss = (-s - beta * entropy).mean()
    c_loss = ((ret - v.reshape(M)) ** 2).mean()
    return a_loss, c_loss


def ppo_loss_grad_factored_reference(logits, v, ret, adv, logp_old, actions, n_heads, n_act=N_ACT, beta=ENTROPY_BETA, clip=0.2):
    """The closed-form gradient uavagent_ppo_loss_grad_factored implements, in PyTorch (dtype of logits): loss_grad_factored_reference with
    its td replaced by w = clipped ? 0 : rho adv in the chosen-action term and td = ret - v in the critic's:
        gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - [j == d_b] w / (p_{d_b} + e);   d a_loss / d z_j = p_j (gp_j - sum_i p_i gp_i) / M
    -> (dlogits [M, B*A], dv [M], dbias [B*A], (a_loss, c_loss, sum(dv), clip_fraction, mean(logp_old - logp)))."""
    M, B, A = logits.shape[0], int(n_heads), int(n_act)
    z = logits.reshape(M, B, A)
    p = torch.softmax(z, dim=2)
    d = joint_to_digits(actions.reshape(-1).clamp(0, A ** B - 1), B, A)
    adv, ret, logp_old = (t.reshape(M).to(z.dtype) for t in (adv, ret, logp_old))
    lp = torch.log(p + 1e-5)
    hot = torch.zeros_like(p).scatter_(2, d.unsqueeze(2), 1.0)
    logp = logp_factored(p, actions)                                            # the one statement of logp: unchanged logits give rho == 1
    rho = torch.exp(logp - logp_old)
    clipped = _ppo_clipped(rho, adv, clip)
    w =torch.where(clipped, torch.zeros_like(rho), rho * adv)
    gp = beta * (lp + p / (p + 1e-5)) - hot * (w.reshape(M, 1, 1) / (p + 1e-5))
    dot = (p * gp).sum(dim=2, keepdim=True)
    dz = (p * (gp - dot) / M).reshape(M, B * A)
    td = ret - v.reshape(M).to(z.dtype)
    dv = -2.0 * td / M
    h = -(p * lp).sum(dim=(1, 2))
    s = torch.where(clipped, rho.clamp(1.0 - clip, 1.0 + clip), rho) * adv
    a_loss = (-s - beta * h).mean()
    return dz, dv, dz.sum(dim=0), (a_loss, (td ** 2).mean(), dv.sum(), float(clipped.double().mean()), (logp_old - logp).mean())


# ---- imitation: the cross entropy against a target distribution per head in place of the chosen-action term ----------
def onehot_targets(labels, n_heads, n_act=N_ACT, dtype=torch.float64):
    """JOINT actions int64 [M] (clamped to [0, n_act^n_heads - 1], the kernel's clamp) -> q [M, n_heads, n_act], the one-hot of each digit."""
    d = joint_to_digits(torch.as_tensor(labels).reshape(-1).clamp(0, int(n_act) ** int(n_heads) - 1), n_heads, n_act)
    return torch.zeros(d.shape + (int(n_act),), dtype=dtype, device=d.device).scatter_(2, d.unsqueeze(2), 1.0)


def soft_targets(table, tau):
    """Reward table [..., n_act] (float64: coordinate_actions(rewards=True) is [N, nBS, 5]) -> q of the same shape,
    q = softmax((t - max t) / tau) over the last axis, in float64: what uavagent_soft_targets_f32 rounds to float32."""
    if not tau > 0 or tau == float("inf"):
        raise ValueError("tau must be finite and > 0")
    t = torch.as_tensor(table, dtype=torch.float64)
    return torch.softmax((t - t.max(dim=-1, keepdim=True).values) * (1.0 / float(tau)), dim=-1)


def greedy_digits(logits):
    """The greedy digit per head of logits [M, B, A], the rule of uavagent_choose_factored_f32(uniforms = NULL): the first index whose value
    no other exceeds (strict >), a NaN never wins, an all-NaN head gives 0."""
    M, B, A = logits.shape
    bv = torch.zeros((M, B), dtype=logits.dtype, device=logits.device)
    bi = torch.full((M, B), -1, dtype=torch.int64, device=logits.device)
    for j in range(A):
        x = logits[:, :, j]
        take = (x == x) & ((bi < 0) | (x > bv))
        bv, bi = torch.where(take, x, bv), torch.where(take, torch.full_like(bi, j), bi)
    return bi.clamp(min=0)


def agreement(logits, q):
    """The fraction of (row, head) pairs whose greedy digit is the first maximum of q [M, B, A] (a float)."""
    return float((greedy_digits(logits.detach()) == greedy_digits(q)).double().mean())


def imitation_losses_factored(head_prob, v, q, v_target, beta=ENTROPY_BETA):
    """(a_loss, c_loss) of the supervised phase.  head_prob and q [M, B, A] (sum_j q_bj = 1), v and v_target [M, 1].  With e = 1e-5:
        X_b = -sum_j q_bj log(p_bj + e);  H_b = -sum_j p_bj log(p_bj + e);  a_loss = mean_rows sum_b (X_b - beta H_b)
    and the critic's loss of a2c_losses_factored: c_loss = mean((v_target - v)^2).  With q = onehot(d) the actor's loss is
    a2c_losses_factored's at td = 1."""
    p = _heads(head_prob)
    td = v_target - v
    c_loss = (td ** 2).mean()
    lp = torch.log(p + 1e-5)
    x = -(q.to(p.dtype) * lp).sum(dim=(1, 2))
    h = -(p * lp).sum(dim=(1, 2))
    return (x - beta * h).mean(), c_loss


def imitation_loss_grad_factored_reference(logits, v, v_target, n_heads, n_act=N_ACT, beta=ENTROPY_BETA, labels=None, targets=None):
    """The closed-form gradient uavagent_imitation_loss_grad_factored implements, in PyTorch (dtype of logits): loss_grad_factored_reference
    with the chosen-action term generalised to a target distribution q per head -- labels (JOINT actions [M], q = their one-hot) or targets
    [M, B * A]:   gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - q_j / (p_j + e);   d a_loss / d z_j = p_j (gp_j - sum_i p_i gp_i) / M;
    d c_loss / d v = -2 td / M.   -> (dlogits [M, B*A], dv [M], dbias [B*A], (a_loss, c_loss, sum(dv), agreement))."""
    if (labels is None) == (targets is None):
        raise ValueError("exactly one of labels and targets must be given")
    M, B, A = logits.shape[0], int(n_heads), int(n_act)
    z = logits.reshape(M, B, A)
    q = onehot_targets(labels, B, A, z.dtype) if labels is not None else targets.reshape(M, B, A).to(z.dtype)
    p = torch.softmax(z, dim=2)
    td = (v_target.reshape(M) - v.reshape(M)).to(z.dtype)
    lp = torch.log(p + 1e-5)
    gp = beta * (lp + p / (p + 1e-5)) - q / (p + 1e-5)
    dot = (p * gp).sum(dim=2, keepdim=True)
    dz = (p * (gp - dot) / M).reshape(M, B * A)
    dv = -2.0 * td / M
    a_loss = (-(q * lp).sum(dim=(1, 2)) + beta * (p * lp).sum(dim=(1, 2))).mean()
    return dz, dv, dz.sum(dim=0), (a_loss, (td ** 2).mean(), dv.sum(), agreement(z, q))


class FactoredCnnACNet(CnnACNet):
    """CnnACNet(n_bs, grid_n, n_bs * n_act) whose policy output is read as n_bs heads of n_act logits.  Parameter keys and shapes are
    CnnACNet's (the head is [100, n_bs * n_act]), so agent.save_actor_npz / load_actor_npz serve it; ``forward``, ``actor_only`` and
    ``forward_reference`` return the per-head probabilities [M, n_bs * n_act] (every run of n_act sums to 1)."""

    factored = True

    def __init__(self, n_bs, grid_n, n_act=N_ACT, seed=6):
        super().__init__(n_bs, grid_n, int(n_bs) * int(n_act), seed=seed)
        self.n_heads, self.n_act = int(n_bs), int(n_act)
        self.joint_actions = self.n_act ** self.n_heads

    def _head_softmax(self, logits):
        M = logits.shape[0]
        return torch.softmax(logits.reshape(M, self.n_heads, self.n_act), dim=-1).reshape(M, self.n_action)

    def forward_reference(self, dense_obs):
        ha, hc = self._trunk_reference(dense_obs, "a"), self._trunk_reference(dense_obs, "c")
        return self._head_softmax(ha @ self.a_ap_k + self.a_ap_b), hc @ self.c_v_k + self.c_v_b

    def forward(self, idx):
        if idx.is_cuda:
            ha, hc = _trunks_cuda(self, idx, ("a", "c"))
            return self._head_softmax(_logits_cuda(self, ha)), _value_cuda(self, hc)
        return self.forward_reference(self._dense(idx))

    def actor_only(self, idx):
        if idx.is_cuda:
            (ha,) = _trunks_cuda(self, idx, ("a",))
            return self._head_softmax(_logits_cuda(self, ha))
        ha = self._trunk_reference(self._dense(idx), "a")
        return self._head_softmax(ha @ self.a_ap_k + self.a_ap_b)


class FactoredCnnA2CRunner(CnnA2CRunner):
    """CnnA2CRunner with the factorised head: one uniform per (step, env, UAV), the draw by uavagent_choose_factored_f32 (GPU) or
    sample_actions_factored (CPU), act_buf holding JOINT actions as the env takes them, and the factored loss in both update forms.
    Serves every shape the env and the CNN's conv1 gather serve (up to 16 UAVs, 256 nodes)."""

    NET_KIND = "cnn-factored"

    def __init__(self, env, net=None, rollout=50, *, seed=6, mask_margin=None, **kw):
        if mask_margin is not None:
            raise ValueError("FactoredCnnA2CRunner: mask_margin serves the factored MLP learner (FactoredA2CRunner) only")
        if net is None:
            net = FactoredCnnACNet(env.nBS, env.grid_n, env.N_ACT, seed=seed)
        if not isinstance(net, FactoredCnnACNet):
            raise TypeError("FactoredCnnA2CRunner trains a FactoredCnnACNet")
        if net.n_heads != env.nBS or net.joint_actions != env.action_space_dim:
            raise ValueError("the net has %d heads of %d actions, the env %d UAVs and %d joint actions" % (
                net.n_heads, net.n_act, env.nBS, env.action_space_dim))
        super().__init__(env, net=net, rollout=rollout, seed=seed, **kw)
        self.u_buf = torch.empty((self.T, env.n_envs, net.n_heads), dtype=torch.float32, device=self.dev)

    def _draw(self, logits, t):
        from . import _agent_capi as A

        A.choose_factored(logits, self.u_buf[t], self.net.n_heads, self.net.n_act, out=self.act_buf[t])

    def _draw_reference(self, t):
        net = self.net
        prob = net.actor_only(self.idx_buf[t]).reshape(-1, net.n_heads, net.n_act)
        return sample_actions_factored(prob, self.u_buf[t])

    def _loss_workspace(self):
        from . import _agent_capi as A

        return A.loss_grad_factored_workspace(self.net.n_heads, self.net.n_act, self.dev)

    def _loss_grad(self, logits, v, target, actions, dv, dbias, loss, ws):
        from . import _agent_capi as A

        A.a2c_loss_grad_factored(logits, v, target, actions, self.net.n_heads, self.net.n_act, self.beta, dv, dbias, loss, ws)

    def _losses(self, a_prob, v, actions, v_target):
        net = self.net
        return a2c_losses_factored(a_prob.reshape(-1, net.n_heads, net.n_act), v, actions, v_target, self.beta)


class FactoredACNet(ACNet):
    """ACNet(n_state, n_bs * n_act) whose policy output is read as n_bs heads of n_act logits.  Parameter keys and shapes are ACNet's (the
    head is [200, n_bs * n_act]), so agent.save_actor_npz / load_actor_npz serve it; ``forward``, ``actor_only`` and ``forward_dense`` return
    the per-head probabilities [M, n_bs * n_act] (every run of n_act sums to 1)."""

    factored = True

    def __init__(self, n_state, n_bs, n_act=N_ACT, hidden=HIDDEN, seed=6):
        super().__init__(n_state, int(n_bs) * int(n_act), hidden=hidden, seed=seed)
        self.n_heads, self.n_act = int(n_bs), int(n_act)
        self.joint_actions = self.n_act ** self.n_heads

    allowed = None      # bool [M, n_heads, n_act] while a masked reference pass runs (FactoredA2CRunner._masked): the digits not in it count as -inf

    def _policy_prob(self, logits):
        M = logits.shape[0]
        z = logits.reshape(M, self.n_heads, self.n_act)
        if self.allowed is not None:
            z = mask_logits(z, self.allowed)
        return torch.softmax(z, dim=-1).reshape(M, self.n_action)


class FactoredA2CRunner(A2CRunner):
    """A2CRunner with the factorised head: one uniform per (step, env, UAV), the draw by uavagent_choose_factored_f32 (GPU) or
    sample_actions_factored (CPU), act_buf holding JOINT actions as the env takes them, the factored loss in both update forms.  Up to 256
    observation nodes (16 UAV x 200 UE): above 64 the first layer -- from the index list, from the observation (``fused_obs``) and its table
    gradient -- runs on libuavagent's wide kernels; at 64 nodes or fewer on the ones A2CRunner uses.  The rollout step is first layer ->
    gemm_rows -> gemm_rows -> choose_factored -> env step, in the captured graph.  The fused actor head, the pipelined halves and the
    persistent rollout are built around 577-640 logits and 4 UAVs: they stay off here."""

    NET_KIND = "mlp-factored"
    FUSED_OBS_MAX_NODES = 256     # uavagent_first_layer_wide_from_obs_f32
    mask_margin = None            # the move mask's margin; None = no masking
    _mask_idx = None              # while update_fused / _ppo_prepare run with a mask: the index rows [M, K] of the logits at hand

    def __init__(self, env, net=None, rollout=50, *, seed=6, mask_margin=None, **kw):
        # mask_margin: None = no masking, exactly the launches there were; an integer m >= 0 = the digits
        # heuristics.move_mask forbids under margin m leave the policy's support -- one uavagent_mask_move_logits_f32 launch in front of
        # the draw (rollout, inside the captured graph), of the loss gradient and of PPO's log pi_old (update), from the batch's own idx rows
        self.mask_margin = check_mask_margin(mask_margin)
        if self.mask_margin is not None and int(env.N_ACT) != 5:
            raise ValueError("FactoredA2CRunner: mask_margin is stated for n_act == 5 (four moves and stay)")
        self._mask_consts = None      # (grid_n, bs_step, min_bs_dist) of the env's config
        if self.mask_margin is not None:
            self._mask_consts = (int(env.grid_n), int(env.cfg.bs_step), int(env.cfg.min_bs_dist))
        if net is None:
            net = FactoredACNet((env.nBS + 1) * env.grid_n * env.grid_n, env.nBS, env.N_ACT, seed=seed)
        if not isinstance(net, FactoredACNet):
            raise TypeError("FactoredA2CRunner trains a FactoredACNet")
        if net.n_heads != env.nBS or net.joint_actions != env.action_space_dim:
            raise ValueError("the net has %d heads of %d actions, the env %d UAVs and %d joint actions" % (
                net.n_heads, net.n_act, env.nBS, env.action_space_dim))
        for k in ("fused_head", "pipeline_halves", "persistent_rollout"):
            if kw.get(k) not in (None, False):
                raise ValueError("FactoredA2CRunner: %s serves the joint head of 4 UAVs only" % k)
            kw[k] = False
        super().__init__(env, net=net, rollout=rollout, seed=seed, **kw)
        self.u_buf = torch.empty((self.T, env.n_envs, net.n_heads), dtype=torch.float32, device=self.dev)
        self._imit = None             # "hard" / "soft" while imitate_rollout's update runs: the loss hooks answer with the imitation form
        self._imit_marks = None       # tools/bench_imitate.py: a list makes the imitation rollout record (phase, event) pairs into it

    def _gather_kernels(self):
        from . import _agent_capi as A

        if self.idx_buf.shape[2] <= A.NARROW_NODES:
            return super()._gather_kernels()
        return A.sparse_rows_sum_wide, A.first_layer_from_obs_wide, A.rows_grad_sort_wide, A.rows_grad_sums_wide

    # ---- move masking ---------------------------------------------------------------------------------------
    def _mask(self, logits, idx):
        """The masking pass on ``logits`` (GPU, in place) from the index rows ``idx`` they were computed from."""
        from . import _agent_capi as A

        G, s, D = self._mask_consts
        A.mask_move_logits(logits, self.net.n_heads, G, s, D, self.mask_margin, idx=idx)

    def allowed(self, idx):
        """bool [M, n_heads, 5]: the digits the mask allows for the index rows ``idx`` (the PyTorch statement; all True without a mask)."""
        if self.mask_margin is None:
            return torch.ones((idx.shape[0], self.net.n_heads, self.net.n_act), dtype=torch.bool, device=idx.device)
        G, s, D = self._mask_consts
        return allowed_from_idx(idx, self.net.n_heads, G, s, D, self.mask_margin)

    def _masked(self, fn, idx):
        """fn(idx) of the net with the policy output under the mask of ``idx`` (the reference paths)."""
        if self.mask_margin is None:
            return fn(idx)
        self.net.allowed = self.allowed(idx)
        try:
            return fn(idx)
        finally:
            self.net.allowed = None

    def _actor_prob(self, idx):
        return self._masked(self.net.actor_only, idx)

    def _reference_forward(self, idx):
        return self._masked(self.net, idx)

    def _with_mask_idx(self, fn, idx_buf, *args, **kw):
        if self.mask_margin is None:
            return fn(idx_buf, *args, **kw)
        self._mask_idx = idx_buf.reshape(-1, idx_buf.shape[2])
        try:
            return fn(idx_buf, *args, **kw)
        finally:
            self._mask_idx = None

    def update_fused(self, idx_buf, act_buf, rew_buf, boot):
        return self._with_mask_idx(super().update_fused, idx_buf, act_buf, rew_buf, boot)

    def _ppo_prepare(self, idx_buf, act_buf, rew_buf, boot, lam, normalize_adv, fused):
        return self._with_mask_idx(super()._ppo_prepare, idx_buf, act_buf, rew_buf, boot, lam, normalize_adv, fused)

    def _draw(self, logits, t, lo, hi):
        from . import _agent_capi as A

        if self.mask_margin is not None:      # (fused_obs: the first layer of this step has just written idx_buf[t])
            self._mask(logits, self.idx_buf[t][lo:hi])
        A.choose_factored(logits, self.u_buf[t][lo:hi], self.net.n_heads, self.net.n_act, out=self.act_buf[t][lo:hi])

    def _draw_reference(self, t):
        net = self.net
        prob = self._actor_prob(self.idx_buf[t]).reshape(-1, net.n_heads, net.n_act)
        return sample_actions_factored(prob, self.u_buf[t])

    def _loss_workspace(self):
        from . import _agent_capi as A

        return A.loss_grad_factored_workspace(self.net.n_heads, self.net.n_act, self.dev)

    def _logp(self, x, actions, fused):
        net = self.net
        if fused:
            from . import _agent_capi as A

            if self._mask_idx is not None:    # the recomputed logits of _ppo_prepare (the rollout's own are masked already: twice is once)
                self._mask(x, self._mask_idx)
            return A.logp_factored(x, actions, net.n_heads, net.n_act)
        return logp_factored(x.reshape(-1, net.n_heads, net.n_act), actions)

    def _loss_grad(self, logits, v, target, actions, dv, dbias, loss, ws):
        from . import _agent_capi as A

        net = self.net
        if self._mask_idx is not None:
            self._mask(logits, self._mask_idx)
        if self._ppo is not None:      # ``target`` (the n-step returns update_fused computed) is not used: the batch's GAE returns take its place
            s = self._ppo
            A.ppo_loss_grad_factored(logits, v, s["ret"], s["adv"], s["logp_old"], actions, net.n_heads, net.n_act, self.beta, s["clip"], dv,
                                     dbias, loss, self._upd["ws_ppo"])
        elif self._imit is None:
            A.a2c_loss_grad_factored(logits, v, target, actions, net.n_heads, net.n_act, self.beta, dv, dbias, loss, ws)
        else:      # ``actions`` are the teacher's labels; with soft targets q_buf takes their place
            soft = self._imit == "soft"
            A.imitation_loss_grad_factored(logits, v, target, net.n_heads, net.n_act, self.beta, dv, dbias, loss, self._upd["ws_imit"],
                                           labels=None if soft else actions, targets=self.q_buf.view(-1, net.n_action) if soft else None)

    def _losses(self, a_prob, v, actions, v_target):
        net = self.net
        prob = a_prob.reshape(-1, net.n_heads, net.n_act)
        if self._ppo is not None:
            return self._ppo_chunk(prob, v, actions, ppo_losses_factored)
        if self._imit is None:
            return a2c_losses_factored(prob, v, actions, v_target, self.beta)
        # update_reference hands its chunks over in row order: the cursor finds the chunk's rows of q_buf
        n, lo = prob.shape[0], self._imit_cursor
        self._imit_cursor = lo + n
        if self._imit == "soft":
            q = self.q_buf.view(-1, net.n_heads, net.n_act)[lo:lo + n]
        else:
            q = onehot_targets(actions, net.n_heads, net.n_act, prob.dtype)
        self._imit_agree += agreement(prob, q) * n             # (the softmax keeps the order of the logits: their greedy digits)
        return imitation_losses_factored(prob, v, q, v_target, self.beta)

    def _ensure_update_buffers(self, M, K):
        from . import _agent_capi as A

        b = super()._ensure_update_buffers(M, K)
        if "ws_imit" not in b:      # behind the A2C kernel's three sums the imitation kernel writes a fourth (the agreement), the PPO kernel two
            b["loss"] = torch.zeros(5, dtype=torch.float64, device=self.dev)
            b["ws_imit"] = A.imitation_loss_grad_workspace(self.net.n_heads, self.net.n_act, self.dev)
            b["ws_ppo"] = A.ppo_loss_grad_workspace(self.net.n_heads, self.net.n_act, self.dev)
        return b

    def state_dict(self):
        sd = super().state_dict()
        sd["net"] = self.NET_KIND
        if self.mask_margin is not None:      # (without a mask the dict keeps exactly the keys it had)
            sd["mask_margin"] = self.mask_margin
        return sd

    def load_state_dict(self, sd):
        if sd.get("mask_margin") != self.mask_margin:
            raise ValueError("checkpoint was written with mask_margin %r, this runner masks with %r" % (sd.get("mask_margin"), self.mask_margin))
        super().load_state_dict(sd)

    # ---- the imitation warm start.  Self-contained: what it needs of the runner is collect()'s pieces (_first_layer,
    # _policy / _draw_reference, _end_rollout), update() and the two loss hooks above. -----------------------------------------------------
    TEACHERS = ("coordinate", "search", "gradient")

    def _imitation_buffers(self, soft):
        N, T, net = self.env.n_envs, self.T, self.net
        if getattr(self, "label_buf", None) is None:
            self.label_buf = torch.empty((T, N), dtype=torch.int64, device=self.dev)       # the teacher's decision before step t
            self.step_buf = torch.empty((T, N), dtype=torch.int64, device=self.dev)        # the action step t took
            self.u_mix = torch.empty((T, N), dtype=torch.float32, device=self.dev)
            self.q_buf = None
        if soft and self.q_buf is None:
            self.q_buf = torch.empty((T, N, net.n_action), dtype=torch.float32, device=self.dev)
            self._table_buf = torch.empty((N, net.n_heads, net.n_act), dtype=torch.float64, device=self.dev)

    def _mark(self, phase):
        if self._imit_marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._imit_marks.append((phase, e))

    def _teach(self, teacher, t, tau, shaped=False):
        """The teacher's decision for the state the env is in, into label_buf[t]; with ``tau`` also its soft targets into q_buf[t].
        ``shaped``: the teacher values its candidates under the env's reward spec."""
        env, net = self.env, self.net
        kw = {"shaped": True} if shaped else {}
        if callable(teacher):
            self.label_buf[t].copy_(torch.as_tensor(teacher(env), dtype=torch.int64).reshape(-1))
        elif tau is None:
            getattr(env, teacher + "_actions")(actions_out=self.label_buf[t], **kw)
        else:
            env.coordinate_actions(rewards=True, actions_out=self.label_buf[t], table_out=self._table_buf, **kw)
            self._mark("teacher")
            if self.dev.type == "cuda":
                from . import _agent_capi as A

                A.soft_targets(self._table_buf.view(-1, net.n_action), net.n_heads, net.n_act, tau, out=self.q_buf[t])
            else:
                self.q_buf[t].copy_(soft_targets(self._table_buf, tau).reshape(-1, net.n_action))

    @torch.no_grad()
    def _imitate_collect(self, teacher, mix, tau, shaped=False):
        """collect() with a teacher beside the learner: per step the learner's forward pass and draw (act_buf[t]), the teacher's decision for
        the same state (label_buf[t], q_buf[t]), and the env stepped with the teacher's action where u_mix[t] < mix, else the learner's
        (step_buf[t]).  Eager launches, no host synchronisation inside the loop."""
        env, T, N = self.env, self.T, self.env.n_envs
        self._check_reward_spec()
        self.u_buf.copy_(torch.rand(self.u_buf.shape, device=self.dev, dtype=torch.float32, generator=self.gen))
        self.u_mix.copy_(torch.rand(self.u_mix.shape, device=self.dev, dtype=torch.float32, generator=self.gen))
        from_teacher = self.u_mix < float(mix)
        self._refresh_transposed()
        self.idx_buf[0].copy_(self.idx_buf[T])
        cuda = self.dev.type == "cuda"
        self._mark("start")
        for t in range(T):
            if cuda:
                self._first_layer(t, 0, N)
                self._policy(t, 0, N)
            else:
                self.act_buf[t] = self._draw_reference(t)
            self._mark("learner")
            self._teach(teacher, t, tau, shaped)
            self._mark("teacher" if tau is None else "soft_targets")
            torch.where(from_teacher[t], self.label_buf[t], self.act_buf[t], out=self.step_buf[t])
            env.step(self.step_buf[t], reward_out=self.rew_buf[t])
            self._after_step(t, cuda and self.fused_obs)
            self._mark("env_step")
        done = env.out["done"].bool()
        any_done = bool(done.any())                                                  # (host sync: the rollout's kernels have finished)
        self._fwd_valid = self._fwd is not None
        return self._end_rollout(done, any_done)

    def imitate_rollout(self, teacher="coordinate", mix=0.5, tau=None, shaped_teacher=False):
        """One rollout and one update of the supervised phase: the actor learns the teacher's decisions (cross entropy per UAV, the entropy
        bonus kept) on the states of a trajectory that follows the teacher with probability ``mix`` per (step, env) and the learner's own
        draw otherwise -- mix = 1: behaviour cloning on the teacher's trajectories, mix = 0: DAgger on the learner's own; the critic learns
        the n-step returns of that trajectory as in train_rollout.  ``teacher``: "coordinate", "search" or "gradient" (the env's own
        *_actions call; its refusals pass through) or a callable teacher(env) -> int64 [N] joint actions.  ``tau``: None = hard labels; a
        temperature = soft targets softmax(table / tau) per UAV from the coordinate search's reward table ("coordinate" only).
        ``shaped_teacher``: the "coordinate" / "search" teacher values its candidates under the env's reward spec (``shaped=True`` of the
        env's call; the soft targets then come from the shaped table) -- refused without a spec, for "gradient" (it uses no reward) and for
        a callable.
        Returns update()'s stats with ``agreement`` added: the fraction of (sample, UAV) pairs whose greedy digit is the teacher's."""
        if self.mask_margin is not None:
            raise ValueError("imitate_rollout: imitation under a move mask is not built (a teacher's label may be a masked digit); "
                             "use a runner with mask_margin=None")
        if not callable(teacher) and teacher not in self.TEACHERS:
            raise ValueError("teacher must be one of %s or a callable teacher(env) -> int64 [n_envs]" % (self.TEACHERS,))
        if shaped_teacher:
            if callable(teacher) or teacher not in ("coordinate", "search"):
                raise ValueError("shaped_teacher needs a teacher that values a reward: 'coordinate' or 'search'")
            if getattr(self.env, "reward", None) is None:
                raise ValueError("shaped_teacher needs a reward spec on the env (set_reward)")
        if tau is not None:
            if teacher != "coordinate":
                raise ValueError("soft targets (tau) need the teacher's reward table: teacher='coordinate' only")
            if not float(tau) > 0 or float(tau) == float("inf"):
                raise ValueError("tau must be finite and > 0")
        if not 0.0 <= float(mix) <= 1.0:
            raise ValueError("mix must be in [0, 1]")
        self._imitation_buffers(tau is not None)
        idx, _, rew, boot = self._imitate_collect(teacher, mix, tau, bool(shaped_teacher))
        return self._with_episodes(self.imitate_update(idx, rew, boot, soft=tau is not None))

    def imitate_update(self, idx_buf, rew_buf, boot, soft=False, fused=None):
        """update() in imitation mode on the batch the last imitation rollout left: the teacher's label_buf (``soft``: q_buf) takes the
        place of act_buf, the loss hooks answer with the imitation form, everything else is the A2C update as it stands.  ``fused``:
        None = update()'s choice, True / False = update_fused / update_reference.  Returns the stats with ``agreement`` added."""
        if fused is None:
            fused = self.fused_update and self.dev.type == "cuda"
        self._imit, self._imit_cursor, self._imit_agree = ("soft" if soft else "hard"), 0, 0.0
        try:
            stats = (self.update_fused if fused else self.update_reference)(idx_buf, self.label_buf, rew_buf, boot)
            stats["agreement"] = float(self._upd["loss"][3]) if fused else self._imit_agree / self.label_buf.numel()
        finally:
            self._imit = None
        return stats
