"""MLP actor-critic + synchronous A2C for the batched env, in PyTorch-ROCm (SURVEY.md section 8 f, row 1).

Restated from the reference's TF1 code, which cannot run here (no tensorflow): **parity unpinned** -- the tests
compare against NumPy restatements of the same formulas, not against TF outputs.
  network   main.py:143-156   two separate trunks  N_S -> 200 relu6 -> 200 relu6 -> {N_A softmax | 1}
            weights N(0, 0.1) (main.py:145), biases 0 (tf.layers.dense default)
  loss      main.py:64-74     td = v_target - v;  c_loss = mean(td^2);
                              a_loss = mean(-(log(p[a] + 1e-5) * stopgrad(td) + beta * H)),  H = -sum p log(p + 1e-5)
  optimiser main.py:300-301   two tf.train.RMSPropOptimizer(lr=1e-4): decay 0.9, momentum 0, epsilon 1e-10 INSIDE
                              the sqrt, mean-square accumulator initialised to ONES (TF1 semantics)
  rollout   a2c_single_thread.py:107-133,153-186   T-step rollouts, n-step returns with gamma = 0.9 bootstrapped
                              from v(s_T) (0 when done), one update per rollout over all workers' samples

MI355X-side design: the observation is a count map with at most U + B non-zero cells (mobile_env.py:169-170), so
the 50000 x 200 first layer is a gather-sum of weight rows over the COMPACT observation the env kernel already
writes (ue_xy, serving, bs_xy) -- no dense (N, B+1, G, G) tensor is ever materialised on the training path.
Gradients are synchronised with one flat all-reduce per update (RCCL over xGMI when launched one process per GPU).
"""

import math

import torch
import torch.nn.functional as F

GAMMA = 0.9           # main.py:20
ENTROPY_BETA = 0.001  # main.py:21
LR_A = 1e-4           # main.py:22
LR_C = 1e-4           # main.py:23
HIDDEN = 200          # main.py:147-148


def obs_to_indices(obs, grid_n, n_bs):
    """Compact observation -> flat indices of the non-zero cells of the reference's raveled state
    (np.ravel of (nBS+1, G, G), main.py:190,202):  plane 0 = UAV cells, plane 1+b = UEs served by UAV b."""
    G = int(grid_n)
    ue = obs["ue_xy"].long()
    bs = obs["bs_xy"].long()
    srv = obs["serving"].long()
    ue_idx = (1 + srv) * (G * G) + ue[..., 0] * G + ue[..., 1]
    bs_idx = bs[..., 0] * G + bs[..., 1]
    # A walker exactly on x == G or y == G (measure zero; the reference raises IndexError there) has no cell in
    # the G x G planes: its entry becomes -1 = "no row", as obs_cell() does for the dense tensor, instead of aliasing the next
    # row / plane.  Both first-layer implementations skip negative indices.
    ue_ok = ((ue >= 0) & (ue < G)).all(dim=-1)
    ue_idx = torch.where(ue_ok, ue_idx, torch.full_like(ue_idx, -1))
    return torch.cat([bs_idx, ue_idx], dim=-1)          # [N, B + U]; duplicates add, like the count map


def first_layer_reference(idx, w_a, b_a, w_c=None, b_c=None):
    """The sparse first layer in plain PyTorch: (h_a, h_c), h = sum_k W[idx[:, k]] + b.  Reference implementation of the HIP
    kernel (tests/test_agent_kernel_gpu.py) and the path CPU tensors take."""
    keep = (idx >= 0).to(w_a.dtype)                     # -1 = "no row" (obs_to_indices): weight 0
    safe = idx.clamp(min=0)
    ha = F.embedding_bag(safe, w_a, per_sample_weights=keep, mode="sum") + b_a
    hc = None if w_c is None else F.embedding_bag(safe, w_c, per_sample_weights=keep, mode="sum") + b_c
    return ha, hc


def sparse_first_layer(idx, w_a, b_a, w_c=None, b_c=None):
    """x @ W + b of main.py:147-148,153 for the raveled state with its nBS + nUE non-zero entries given as row indices.
    CUDA tensors: one launch of libuavagent.so for both tables (they share idx), an error if the library is missing."""
    if idx.is_cuda:
        from ._agent_capi import sparse_first_layer_cuda

        return sparse_first_layer_cuda(idx, w_a, b_a, w_c, b_c)
    return first_layer_reference(idx, w_a, b_a, w_c, b_c)


class ACNet(torch.nn.Module):
    """Actor and critic trunks of main.py:143-156.  The first layers are stored as [N_S, 200] tables so that the
    sparse path is an embedding-bag sum; ``forward_dense`` is the textbook matmul on the raveled dense state."""

    def __init__(self, n_state, n_action, hidden=HIDDEN, seed=6):
        super().__init__()
        g = torch.Generator().manual_seed(int(seed))    # TENSOR_SEED = 6 (main.py:26); not TF's stream
        def w(*shape):
            return torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.1)   # random_normal_initializer(0, .1)
        def b(n):
            return torch.nn.Parameter(torch.zeros(n))
        self.n_state, self.n_action = int(n_state), int(n_action)
        self.a_w1, self.a_b1 = w(n_state, hidden), b(hidden)
        self.a_w2, self.a_b2 = w(hidden, hidden), b(hidden)
        self.a_w3, self.a_b3 = w(hidden, n_action), b(n_action)
        self.c_w1, self.c_b1 = w(n_state, hidden), b(hidden)
        self.c_w2, self.c_b2 = w(hidden, hidden), b(hidden)
        self.c_w3, self.c_b3 = w(hidden, 1), b(1)

    def actor_params(self):
        return [self.a_w1, self.a_b1, self.a_w2, self.a_b2, self.a_w3, self.a_b3]

    def critic_params(self):
        return [self.c_w1, self.c_b1, self.c_w2, self.c_b2, self.c_w3, self.c_b3]

    def _policy_prob(self, logits):
        """The policy output from the head's logits: one softmax over the joint actions (factored.FactoredACNet: one per UAV)."""
        return torch.softmax(logits, dim=-1)

    def _heads(self, ha, hc):
        ha = F.relu6(F.relu6(ha) @ self.a_w2 + self.a_b2)
        hc = F.relu6(F.relu6(hc) @ self.c_w2 + self.c_b2)
        a_prob = self._policy_prob(ha @ self.a_w3 + self.a_b3)
        v = hc @ self.c_w3 + self.c_b3
        return a_prob, v

    def forward(self, idx):
        """idx: int64 [M, K] flat indices of the non-zero cells (obs_to_indices)."""
        ha, hc = sparse_first_layer(idx, self.a_w1, self.a_b1, self.c_w1, self.c_b1)
        return self._heads(ha, hc)

    def actor_only(self, idx):
        ha, _ = sparse_first_layer(idx, self.a_w1, self.a_b1)
        ha = F.relu6(F.relu6(ha) @ self.a_w2 + self.a_b2)
        return self._policy_prob(ha @ self.a_w3 + self.a_b3)

    def critic_only(self, idx):
        hc, _ = sparse_first_layer(idx, self.c_w1, self.c_b1)
        hc = F.relu6(F.relu6(hc) @ self.c_w2 + self.c_b2)
        return hc @ self.c_w3 + self.c_b3

    def forward_dense(self, s):
        """s: float [M, N_S], the raveled (nBS+1, G, G) state exactly as the reference feeds it (main.py:190)."""
        return self._heads(s @ self.a_w1 + self.a_b1, s @ self.c_w1 + self.c_b1)


def a2c_losses(a_prob, v, actions, v_target, beta=ENTROPY_BETA):
    """(a_loss, c_loss) of main.py:64-74."""
    td = v_target - v                                                     # :64
    c_loss = (td ** 2).mean()                                             # :66
    log_prob = torch.log(a_prob.gather(1, actions.view(-1, 1)) + 1e-5)    # :69
    exp_v = log_prob * td.detach()                                        # :70
    entropy = -(a_prob * torch.log(a_prob + 1e-5)).sum(dim=1, keepdim=True)  # :71-72
    a_loss = (-(beta * entropy + exp_v)).mean()                           # :73-74
    return a_loss, c_loss


# ---- PPO (DESIGN.md sections 22 and 23): GAE(lambda) advantages and the clipped surrogate in place of the chosen-action term ----------------
def gae_reference(rewards, values, bootstrap, gamma, lam):
    """GAE(lambda) as uavagent_gae_f32 computes it, in the dtype of rewards: rewards and values [T, N], bootstrap [N] (0 where the episode
    ended);  delta[t] = r[t] + gamma v[t+1] - v[t] with v[T] := bootstrap;  adv[t] = delta[t] + gamma lam adv[t+1];  ret = adv + v.
    -> (adv, ret).  lam = 1: ret is agent.nstep_returns; lam = 0: adv is the one-step TD error."""
    T = rewards.shape[0]
    values = values.to(rewards.dtype)
    adv, run, next_v = torch.empty_like(rewards), torch.zeros_like(rewards[0]), bootstrap.to(rewards.dtype)
    for t in range(T - 1, -1, -1):
        run = (rewards[t] + gamma * next_v) - values[t] + (gamma * lam) * run
        adv[t] = run
        next_v = values[t]
    return adv, adv + values


def logp_joint(prob, actions):
    """log pi(a | s) = log(p_a + 1e-5) of the actions [M] under prob [M, A] (the kernel's clamp of the actions into [0, A)) -> [M]."""
    A = prob.shape[1]
    return torch.log(prob.gather(1, actions.reshape(-1, 1).clamp(0, A - 1)).squeeze(1) + 1e-5)


def _ppo_clipped(rho, adv, clip):
    return ((adv > 0) & (rho > 1.0 + clip)) | ((adv < 0) & (rho < 1.0 - clip))


def ppo_losses(prob, v, actions, adv, ret, logp_old, beta=ENTROPY_BETA, clip=0.2):
    """(a_loss, c_loss) of PPO for one softmax over the joint actions, differentiable.  prob [M, A], v [M, 1], actions [M]; adv, ret and
    logp_old [M] (or [M, 1]) are constants.  rho = exp(logp - logp_old); a row is clipped when (adv > 0 and rho > 1 + clip) or (adv < 0 and
    rho < 1 - clip); s = clipped ? clamp(rho, 1 - clip, 1 + clip) adv : rho adv;  a_loss = mean(-s - beta H), H as in a2c_losses;
    c_loss = mean((ret - v)^2)."""
    M = prob.shape[0]
    adv, ret, logp_old = (t.reshape(M).detach().to(prob.dtype) for t in (adv, ret, logp_old))
    rho = torch.exp(logp_joint(prob, actions) - logp_old)
    clipped = _ppo_clipped(rho.detach(), adv, clip)
    s = torch.where(clipped, rho.detach().clamp(1.0 - clip, 1.0 + clip), rho) * adv       # a clipped row is a constant of the parameters
    entropy = -(prob * torch.log(prob + 1e-5)).sum(dim=1)
    a_loss = (-s - beta * entropy).mean()
    c_loss = ((ret - v.reshape(M)) ** 2).mean()
    return a_loss, c_loss


def ppo_loss_grad_reference(logits, v, ret, adv, logp_old, actions, beta=ENTROPY_BETA, clip=0.2):
    """The closed-form gradient uavagent_ppo_loss_grad implements, in PyTorch (dtype of logits): uavagent_a2c_loss_grad's statements with
    its td replaced by w = clipped ? 0 : rho adv in the chosen-action term and td = ret - v in the critic's:
        gp_j = beta (log(p_j + e) + p_j / (p_j + e)) - [j == d] w / (p_d + e);   d a_loss / d z_j = p_j (gp_j - sum_i p_i gp_i) / M
    -> (dlogits [M, A], dv [M], dbias [A], (a_loss, c_loss, sum(dv), clip_fraction, mean(logp_old - logp)))."""
    M, A = logits.shape
    p = torch.softmax(logits, dim=1)
    d = actions.reshape(-1, 1).clamp(0, A - 1)
    adv, ret, logp_old = (t.reshape(M).to(logits.dtype) for t in (adv, ret, logp_old))
    lp = torch.log(p + 1e-5)
    hot = torch.zeros_like(p).scatter_(1, d, 1.0)
    logp = logp_joint(p, actions)                                               # the one statement of logp: unchanged logits give rho == 1
    rho = torch.exp(logp - logp_old)
    clipped = _ppo_clipped(rho, adv, clip)
    w = torch.where(clipped, torch.zeros_like(rho), rho * adv)
    gp = beta * (lp + p / (p + 1e-5)) - hot * (w.reshape(M, 1) / (p + 1e-5))
    dot = (p * gp).sum(dim=1, keepdim=True)
    dz = p * (gp - dot) / M
    td = ret - v.reshape(M).to(logits.dtype)
    dv = -2.0 * td / M
    h = -(p * lp).sum(dim=1)
    s = torch.where(clipped, rho.clamp(1.0 - clip, 1.0 + clip), rho) * adv
    a_loss = (-s - beta * h).mean()
    return dz, dv, dz.sum(dim=0), (a_loss, (td ** 2).mean(), dv.sum(), float(clipped.double().mean()), (logp_old - logp).mean())


class TFRMSProp:
    """tf.train.RMSPropOptimizer(learning_rate) as TF1 implements it (main.py:300-301):
        ms <- decay * ms + (1 - decay) * g^2         (ms initialised to ONES)
        var <- var - lr * g / sqrt(ms + epsilon)     (epsilon = 1e-10 inside the sqrt, momentum = 0)"""

    def __init__(self, params, lr, decay=0.9, eps=1e-10):
        self.params = list(params)
        self.lr, self.decay, self.eps = float(lr), float(decay), float(eps)
        self.ms = [torch.ones_like(p) for p in self.params]

    @torch.no_grad()
    def step(self):
        grads = [p.grad for p in self.params]
        torch._foreach_mul_(self.ms, self.decay)
        torch._foreach_addcmul_(self.ms, grads, grads, value=1.0 - self.decay)
        denom = torch._foreach_add(self.ms, self.eps)
        torch._foreach_sqrt_(denom)
        torch._foreach_addcdiv_(self.params, grads, denom, value=-self.lr)

    def zero_grad(self):
        for p in self.params:
            if p.grad is not None:
                p.grad.zero_()          # keeps FlatParams' gradient views in place

    def state_dict(self):
        return {"ms": [m.clone() for m in self.ms], "lr": self.lr, "decay": self.decay, "eps": self.eps}

    def load_state_dict(self, sd):
        for m, s in zip(self.ms, sd["ms"]):
            m.copy_(s)


class Adam:
    """torch.optim.Adam(lr, betas, eps) without weight decay and amsgrad, on the parameters' .grad (an extension, the
    reference trains with RMSProp only):
        m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;  p <- p - [lr / (1 - b1^t)] m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    The caller holds the step number t = 1, 2, ... (the runner advances it only for steps that were taken)."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8):
        self.params = list(params)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]

    @torch.no_grad()
    def step(self, t):
        b1, b2 = self.betas
        grads = [p.grad for p in self.params]
        torch._foreach_mul_(self.m, b1)
        torch._foreach_add_(self.m, grads, alpha=1.0 - b1)
        torch._foreach_mul_(self.v, b2)
        torch._foreach_addcmul_(self.v, grads, grads, value=1.0 - b2)
        denom = torch._foreach_sqrt(self.v)
        torch._foreach_div_(denom, math.sqrt(1.0 - b2 ** int(t)))
        torch._foreach_add_(denom, self.eps)
        torch._foreach_addcdiv_(self.params, self.m, denom, value=-self.lr / (1.0 - b1 ** int(t)))

    def zero_grad(self):
        for p in self.params:
            if p.grad is not None:
                p.grad.zero_()


def clip_coefficient(g, max_norm):
    """(coef, norm) of torch.nn.utils.clip_grad_norm_ for one flat gradient slice: norm = ||g||_2 summed in float64,
    coef = min(1, max_norm / (norm + 1e-6)).  A norm that is not finite gives coef 1: the caller skips the step."""
    norm = float(g.detach().double().pow(2).sum().sqrt())
    if not math.isfinite(norm):
        return 1.0, norm
    return min(1.0, float(max_norm) / (norm + 1e-6)), norm


def nstep_returns(rewards, bootstrap, gamma=GAMMA):
    """a2c_single_thread.py:176-183: value_estimate = r + gamma * value_estimate, backwards over the rollout.
    rewards [T, N], bootstrap [N] (v(s_T), or 0 where the episode ended) -> targets [T, N]."""
    T = rewards.shape[0]
    out = torch.empty_like(rewards)
    run = bootstrap
    for t in range(T - 1, -1, -1):
        run = rewards[t] + gamma * run
        out[t] = run
    return out


# ---- episodes that end inside a rollout: done [T, N], non-zero where step t ended env n's episode ---------------------
def nstep_returns_done(rewards, done, bootstrap, gamma=GAMMA):
    """nstep_returns with the running return cut at a done step, as uavagent_nstep_returns_done_f32 computes it: the cut is a select of 0
    (``r + gamma * 0``, not ``r``), so a column's segments are nstep_returns of each segment with bootstrap 0, bit for bit."""
    T = rewards.shape[0]
    out = torch.empty_like(rewards)
    run = bootstrap.to(rewards.dtype)
    zero = torch.zeros_like(rewards[0])
    for t in range(T - 1, -1, -1):
        run = rewards[t] + gamma * torch.where(done[t] != 0, zero, run)
        out[t] = run
    return out


def gae_done_reference(rewards, values, done, bootstrap, gamma, lam):
    """gae_reference with the next value and the carried advantage cut at a done step, as uavagent_gae_done_f32 computes it: values[t + 1]
    is then the value of the NEXT episode's first state and does not enter the episode that ended.  -> (adv, ret).
    The constant gamma * lam is formed in the dtype of rewards, as the kernels form it in float32 (gae_reference forms it in float64 and
    rounds then: in float32 the two round apart for some pairs, 0.9 * 0.95 among them, and alike whenever lam is a power of two)."""
    T = rewards.shape[0]
    values = values.to(rewards.dtype)
    adv, run, next_v = torch.empty_like(rewards), torch.zeros_like(rewards[0]), bootstrap.to(rewards.dtype)
    zero = torch.zeros_like(rewards[0])
    gl = float(torch.tensor(gamma, dtype=rewards.dtype) * torch.tensor(lam, dtype=rewards.dtype))
    for t in range(T - 1, -1, -1):
        d = done[t] != 0
        run = (rewards[t] + gamma * torch.where(d, zero, next_v)) - values[t] + gl * torch.where(d, zero, run)
        adv[t] = run
        next_v = values[t]
    return adv, adv + values


def episode_step_reference(reward, done, ep_r, done_row_out, mask_out, fin_sum, fin_cnt):
    """One step of a runner's episode bookkeeping, in place, as uavagent_episode_step_f32 does it: ep_r += reward; the step's done row and
    the mask of the reset that follows := done; where done, the episode's return goes to the per-env totals and ep_r starts again at 0."""
    d = done != 0
    r = ep_r + reward
    done_row_out.copy_(d)
    mask_out.copy_(d)
    fin_sum.copy_(torch.where(d, fin_sum + r.double(), fin_sum))
    fin_cnt.copy_(torch.where(d, fin_cnt + 1, fin_cnt))
    ep_r.copy_(torch.where(d, torch.zeros_like(r), r))


def allreduce_mean_grads(params):
    """One flat all-reduce of every gradient (sum / world size).  With one process per GPU and backend 'nccl' this is
    RCCL over xGMI; a no-op without an initialised process group.  Returns the number of float32 elements reduced."""
    import torch.distributed as dist

    grads = [p.grad for p in params if p.grad is not None]
    n = sum(g.numel() for g in grads)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return n
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    flat.div_(dist.get_world_size())
    off = 0
    for g in grads:
        g.copy_(flat[off:off + g.numel()].view_as(g))
        off += g.numel()
    return n


def sample_actions(prob, generator=None, uniforms=None):
    """One action per row of ``prob`` [N, n_action], the way the reference draws it (main.py:167-168):
    np.random.choice(range(n), p=p) is cdf = p.cumsum(); cdf /= cdf[-1]; searchsorted(cdf, uniform, side='right').
    Same three steps on the device (one uniform per env from ``generator``); a third of the time of torch.multinomial at
    [8192, 625] (tools/profile_a2c.py).  An action of probability 0 is never drawn; the result is always < n_action."""
    cdf = prob.cumsum(dim=1)
    if uniforms is None:
        uniforms = torch.rand((prob.shape[0], 1), device=prob.device, dtype=prob.dtype, generator=generator)
    u = uniforms.reshape(-1, 1).to(prob.dtype) * cdf[:, -1:]
    return torch.searchsorted(cdf, u, right=True).squeeze(1).clamp_(max=prob.shape[1] - 1)


_TUNABLE_DONE = False
_TUNABLE_DIR = None


def freeze_gemm_tuning():
    """Stop TunableOp from TUNING further shapes (the picks already made or loaded stay in use): called by A2CRunner.train_rollout
    after its first rollout + update, so that no later GEMM of the host application -- or of a graph capture -- triggers a timing
    run, and two processes that warmed up on the same shapes keep the same picks.  Returns True when tuning was on and is now off."""
    if _TUNABLE_DONE:
        import torch.cuda.tunable as tun

        tun.tuning_enable(False)
        return True
    return False


def gemm_tuning_is_active():
    """True while TunableOp may still start timing runs for new shapes (enable_gemm_tuning() called, freeze_gemm_tuning() not yet)."""
    if not _TUNABLE_DONE:
        return False
    import torch.cuda.tunable as tun

    return bool(tun.tuning_is_enabled())


def _remove_tunable_dir():
    import shutil

    if _TUNABLE_DIR:
        try:                                  # TunableOp rewrites its results file when the process ends, after this handler:
            import os                         # point it away from the directory that is about to disappear

            import torch.cuda.tunable as tun

            tun.set_filename(os.devnull)
        except Exception:
            pass
        shutil.rmtree(_TUNABLE_DIR, ignore_errors=True)


def enable_gemm_tuning(max_ms=400):
    """Let PyTorch's TunableOp pick the fastest rocBLAS / hipBLASLt solution per GEMM shape.  The defaults run the learner's
    K = 200 shapes and its 409 600-deep weight-gradient reductions at 34-73 TFLOP/s; the tuned picks reach 45-108
    (profiles/r02f_gemm_tunableop.txt: the update's seven large GEMMs 7.3 -> 5.2 ms).  Picks for the BASELINE config 3 shapes ship
    in data/tunableop_gfx950.csv (valid for this image's ROCm / hipBLASLt build: TunableOp checks the versions recorded in the file
    and ignores it otherwise); any other shape is tuned at first use for at most ``max_ms``, outside graph capture (the rollout graph
    is captured after an eager warm-up pass).  Once per process; a no-op without a GPU or without torch.cuda.tunable.
    OPT-IN (A2CRunner(tune_gemms=True); bench.py and tools/train_a2c.py ask for it): it switches TunableOp on for the whole process.
    Bit-identical checkpoint resume holds for the shipped shapes (their picks come from the file); a shape tuned at first use may get
    another pick in another process."""
    global _TUNABLE_DONE, _TUNABLE_DIR
    if _TUNABLE_DONE or not torch.cuda.is_available():
        return _TUNABLE_DONE
    try:
        import atexit
        import os
        import shutil
        import tempfile

        import torch.cuda.tunable as tun

        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "tunableop_gfx950.csv")
        _TUNABLE_DIR = tempfile.mkdtemp(prefix="uavagent_tunable_")
        atexit.register(_remove_tunable_dir)
        dst = os.path.join(_TUNABLE_DIR, "tunableop_results.csv")   # TunableOp rewrites its file at exit
        if os.path.isfile(src):
            shutil.copyfile(src, dst)
        tun.set_filename(dst)
        tun.set_max_tuning_duration(int(max_ms))
        tun.enable(True)
        tun.tuning_enable(True)
        _TUNABLE_DONE = True
    except Exception:                                        # an optional speed-up: never a reason to fail
        _TUNABLE_DONE = False
    return _TUNABLE_DONE


PARAM_ORDER = ("a_w1", "a_b1", "a_w2", "a_b2", "a_w3", "a_b3", "c_w1", "c_b1", "c_w2", "c_b2", "c_w3", "c_b3")
N_ACTOR_PARAMS = 6


class FlatParams:
    """All parameters of an ACNet as views of ONE flat buffer (float32: the parameters' dtype), their gradients as views of a second one and the RMSProp
    mean squares in a third (every view starts on a 256-byte boundary; the padding stays zero).  One buffer = one all-reduce
    with no gather / scatter copies, one fused optimiser launch per trunk, one memset to clear the gradients.  Autograd
    accumulates into the existing .grad views in place, so the reference (autograd) path fills the same buffer."""

    ALIGN = 64   # floats

    def __init__(self, net, adam=False):
        order = getattr(net, "PARAM_ORDER", PARAM_ORDER)              # the net's own order (CnnACNet) or the MLP's
        params = [getattr(net, k) for k in order]
        dev = params[0].device
        offs, off = [], 0
        for p in params:
            offs.append(off)
            off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.n_flat = off
        self.n_real = sum(p.numel() for p in params)
        self.actor_end = offs[getattr(net, "N_ACTOR_PARAMS", N_ACTOR_PARAMS)]   # [0, actor_end) actor trunk, [actor_end, n_flat) critic trunk
        dt = params[0].dtype            # float32; a net made .double() (CPU tests of the reference path) keeps its precision
        self.w = torch.zeros(off, dtype=dt, device=dev)
        self.g = torch.zeros(off, dtype=dt, device=dev)
        self.ms = torch.ones(off, dtype=dt, device=dev)    # TF1: accumulator initialised to ones (main.py:300-301)
        # Adam's moments, only where Adam is the optimiser (two more buffers of the parameters' size); they start at zero
        self.m = torch.zeros(off, dtype=dt, device=dev) if adam else None
        self.v = torch.zeros(off, dtype=dt, device=dev) if adam else None
        self.gv = {}
        with torch.no_grad():
            for k, p, o in zip(order, params, offs):
                view = self.w[o:o + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view
                p.grad = self.g[o:o + p.numel()].view_as(p)
                self.gv[k] = p.grad

    def zero_grad(self):
        self.g.zero_()


class A2CRunner:
    """Synchronous A2C over a BatchedMobiEnv: every env instance plays the role of one of the reference's workers
    (a2c_single_thread.py:113-118), all stepped by one kernel launch per time step.

    On a GPU the rollout loop is ONE hipGraph (per step three kernels: first layer fed from the env's compact observation + the actor's
    head (layer 2, policy head, action draw) + env step) and the update is a hand-derived backward pass on libuavagent's kernels
    (float32 MFMA GEMMs with fused epilogues, loss gradient, table gradient, RMSProp).  Each switch
    (``hip_gemms``, ``fused_head``, ``fused_obs``, ``overlap_allreduce``, ``pipeline_halves``, ``persistent_rollout``) turns on a fused or
    overlapped form where the shapes and the process group allow it; its other setting is the form that still serves the rest, and the tests
    compare the two bit for bit where the arithmetic is the same and to tolerance where it is not.  ``update_reference`` is the same update
    through autograd."""

    def __init__(self, env, net=None, rollout=50, gamma=GAMMA, beta=ENTROPY_BETA, lr_a=LR_A, lr_c=LR_C, seed=6,
                 update_chunk=65536, first_state="obs", collect_launch="graph", fused_update=True, tune_gemms=False, hip_gemms=True,
                 overlap_allreduce=True, fused_head=True, fused_obs=True, pipeline_halves=True, force_exchange=False,
                 persistent_rollout="auto", optimizer="rmsprop", max_grad_norm=None, adam_betas=(0.9, 0.999), adam_eps=1e-8, mask_margin=None):
        if mask_margin is not None:      # (factored.FactoredA2CRunner takes the keyword itself and does not pass it on)
            raise ValueError("%s: mask_margin serves the factored MLP learner (factored.FactoredA2CRunner) only: the joint head's draw is "
                             "fused into its actor-head kernels" % type(self).__name__)
        self._init_common(env, net if net is not None else ACNet(env.observation_space_dim, env.action_space_dim, seed=seed), rollout, gamma,
                          beta, lr_a, lr_c, seed, update_chunk, first_state, tune_gemms, optimizer, max_grad_norm, adam_betas, adam_eps)
        if collect_launch not in ("graph", "eager"):
            raise ValueError("collect_launch must be 'graph' or 'eager'")
        self.collect_launch = collect_launch
        self.fused_update = bool(fused_update)
        # hip_gemms: the update's dense layers through libuavagent's float32 MFMA kernels (csrc/agent_gemm.hip: relu6 masks and bias
        # gradients fused) instead of torch.mm + separate relu6-backward passes.  They are written for the reference's layer widths.
        self.hip_gemms = bool(hip_gemms) and HIDDEN == 200 and self.net.n_action <= 640
        # more than one rank: the critic trunk's gradient (40 MB, first half of the exchange) is all-reduced on a side stream while the
        # actor trunk's backward pass still runs (update_fused, hip_gemms path)
        self.overlap_allreduce = bool(overlap_allreduce)
        # force_exchange (tests): run the gradient exchange -- the collective calls, the side stream, the bucket order -- even when the
        # process group has ONE rank, so that a one-GPU box executes the call sequence an 8-GPU run starts with (backend nccl = RCCL)
        self.force_exchange = bool(force_exchange)
        # fused_head: layer 2, the policy head and the action draw of a rollout step as ONE kernel (uavagent_actor_head_f32)
        self.fused_head = bool(fused_head) and self.hip_gemms and 576 < self.net.n_action <= 640
        # fused_obs: steps 1 .. T-1 of a rollout build their index list inside the first layer's kernel (uavagent_first_layer_from_obs_f32)
        # instead of a separate obs_indices launch after every env step
        self.fused_obs = bool(fused_obs) and env.nBS + env.nUE <= self.FUSED_OBS_MAX_NODES
        self._side = None
        # pipeline_halves (GPU, fused_head + fused_obs): the workers of a2c_single_thread.py:113-118 are independent of each other for a
        # whole rollout, so the batch is cut in two halves that ping-pong on two streams inside the rollout (and inside its captured
        # graph): while the actor's head of one half runs (MFMA / LDS-DMA bound; 16-row workgroups, so that half a batch still gives
        # every CU one), the other half steps its envs (uavenv_step_range) and gathers its first layer (fabric bound, no MFMA).  The
        # two heads never overlap each other (events), which is what keeps the halves out of lockstep.  Same arithmetic per row with the
        # same uniforms: bit-identical to the unsplit rollout.  Measured at 8192 envs x 50 steps, interleaved in one process
        # (profiles/r04i_ab_collect_pipeline_forms.json): 4.40-4.46 ms per rollout against 5.04-5.17 unsplit; three or four parts, or
        # no order between the heads, are slower (every cross-stream edge of the graph costs ~9 us, every node of a two-stream graph ~5).
        # True = when each half still fills the chip (>= 4096 envs), "force" = whenever the batch can be cut (tests).
        self._halves = None
        self._pipe_stream = None
        # (not with a reward spec that terminates: the masked reset behind every step is one launch over the whole batch, and the halves'
        #  step_range calls would need half-masks; the plain per-step loop serves it)
        if pipeline_halves and self.dev.type == "cuda" and self.fused_head and self.fused_obs and self.done_buf is None:
            # the cut lies on a multiple of the head's 16-row tiles (half a batch runs on 16-row workgroups: 8192 envs = 2 x 256 tiles = one
            # workgroup per CU and half)
            mid = min((env.n_envs // 2 + 15) // 16 * 16, env.n_envs)
            if 0 < mid < env.n_envs and (pipeline_halves == "force" or env.n_envs >= 4096):
                self._halves = ((0, mid), (mid, env.n_envs))
        # persistent_rollout (GPU, fused_head + fused_obs, the reference's 4 UAVs and <= 64 UEs): the whole rollout as TWO persistent kernel
        # launches on two streams -- uavagent_actor_head_gated_f32 (the policy) and uavenv_rollout_gated (env step + next observation's first
        # layer) -- that hand 16-env blocks to each other through step counters in device memory (include/uavenv.h has the protocol): no kernel
        # boundary, graph node or cross-stream edge per step any more; each CU hosts one workgroup of either kernel and ping-pongs between the
        # two blocks of its pair.  Same arithmetic per env and step: bit-identical to the other forms.  Every device-side wait is bounded; a
        # timeout makes collect() restore the state the rollout started from and collect it again with the per-step launches.  "auto" = from 4096 envs on; True = whenever the shapes allow (tests); the first
        # collect() proves on a CLONE of the env state that the two kernels do run side by side, and falls back to pipeline_halves if not.
        self._persistent = False
        self._persist_stream = None
        self._persistent_proven = False
        self._persist_same_stream = False            # test hook: both persistent kernels in ONE queue, i.e. never side by side
        self._gate_spin_us = 0                       # test hook: the policy kernel's wait budget; 0 = the library's 2 s
        if (persistent_rollout and self.dev.type == "cuda" and self.fused_head and self.fused_obs and env.nBS == 4 and env.nUE <= 64
                and env.n_envs % 4 == 0 and "cur_sinr_f64" not in env.out and (persistent_rollout is True or env.n_envs >= 4096)
                and getattr(env, "reward", None) is None):   # (the persistent env kernel computes the step's own reward only)
            self._persistent = True
        N, T = env.n_envs, self.T
        # Forward activations of the rollout, kept for the update: between collect() and update() the weights do not change, so
        # relu6(first layer) of both trunks, the actor's second layer and its logits for sample (t, n) ARE the update's forward
        # pass for that sample -- the update only adds the critic's second layer and value head.  (2 GB at 8192 envs x 50 steps.)
        self._fwd = None
        if self.dev.type == "cuda":
            H, NA = HIDDEN, self.net.n_action
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.dev)
            # logits live in rows of LDL = n_action rounded up to 16 floats (625 -> 640) with a ZERO tail: rows start 16-byte aligned,
            # so the update's GEMMs stage them with float4 loads and may read the tail (it multiplies zero weights)
            self._ldl = (NA + 15) // 16 * 16
            self._logits_pad = torch.zeros((T, N, self._ldl), dtype=torch.float32, device=self.dev)
            self._fwd = {"h1a": f(T, N, H), "h1c": f(T, N, H), "h2a": f(T, N, H), "logits": self._logits_pad[:, :, :NA]}
            # the actor's dense layers handed to uavagent_gemm_rows_f32 in its fast form: W^T (k-contiguous rows), the policy head
            # padded to LDL rows / bias entries of zeros (so the tail of every logits row comes out zero); refreshed from the
            # parameters at the start of every collect()
            self._wt = {"a_w2t": f(H, H), "c_w2t": f(H, H), "a_w3t": torch.zeros((self._ldl, H), dtype=torch.float32, device=self.dev),
                        "a_b3p": torch.zeros(self._ldl, dtype=torch.float32, device=self.dev)} if self.hip_gemms else None
        self._fwd_valid = False
        if self._persistent:
            nb = (N + 15) // 16
            self._gate_obs = torch.zeros(nb, dtype=torch.int32, device=self.dev)
            self._gate_act = torch.zeros(nb, dtype=torch.int32, device=self.dev)
            self._gate_claim = torch.zeros(2, dtype=torch.int32, device=self.dev)
            self._persist_state = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=self.dev)
            from . import _agent_capi as _A

            _A.gate_prepare()
        self._graph = None
        self._upd = None              # the update's buffer set in use ...
        self._upd_sets = {}           # ... of the sets kept, by row count (_ensure_update_buffers)

    NET_KIND = "mlp"
    FUSED_OBS_MAX_NODES = 64      # uavagent_first_layer_from_obs_f32: one lane per node (factored.FactoredA2CRunner: the wide form's 256)

    OPTIMIZERS = ("rmsprop", "adam")

    def _init_common(self, env, net, rollout, gamma, beta, lr_a, lr_c, seed, update_chunk, first_state, tune_gemms, optimizer="rmsprop",
                     max_grad_norm=None, adam_betas=(0.9, 0.999), adam_eps=1e-8):
        """What every runner over a BatchedMobiEnv sets up (A2CRunner and cnn_agent.CnnA2CRunner): the net in FlatParams with its two
        optimiser views (TF1 RMSProp, or Adam: DESIGN.md section 24), the rollout buffers, the first state, the episode bookkeeping and the
        action-sampling generator."""
        if optimizer not in self.OPTIMIZERS:
            raise ValueError("optimizer must be one of %s" % (self.OPTIMIZERS,))
        if max_grad_norm is not None and not (math.isfinite(float(max_grad_norm)) and float(max_grad_norm) > 0.0):
            raise ValueError("max_grad_norm must be None or a finite number > 0")
        b1, b2 = (float(x) for x in adam_betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and math.isfinite(float(adam_eps)) and float(adam_eps) > 0.0):
            raise ValueError("adam_betas must lie in [0, 1) and adam_eps must be > 0")
        self.optimizer = optimizer
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.adam_betas, self.adam_eps = (b1, b2), float(adam_eps)
        # Adam's step numbers, (actor, critic): the two networks are two optimisers, and a step that the clip skipped (a gradient norm that
        # is not finite) does not count
        self.opt_step = [0, 0]
        self.env = env
        self.dev = env.device
        # the env's reward spec (BatchedMobiEnv.set_reward) as it is now: it decides the form of the rollout, and a captured rollout
        # graph holds its shaping launches with the spec by value, so collect() refuses an env whose spec has changed since
        self.reward_spec = getattr(env, "reward", None)
        self.gemm_tuning = enable_gemm_tuning() if (tune_gemms and self.dev.type == "cuda") else False
        self.G, self.B = env.grid_n, env.nBS
        self.net = net.to(self.dev)
        adam = optimizer == "adam"
        self.flat = FlatParams(self.net, adam=adam)
        self.lr_a, self.lr_c = float(lr_a), float(lr_c)
        # reference path only; both share FlatParams' accumulators
        if adam:
            self.opt_a = Adam(self.net.actor_params(), lr_a, self.adam_betas, self.adam_eps)
            self.opt_c = Adam(self.net.critic_params(), lr_c, self.adam_betas, self.adam_eps)
        else:
            self.opt_a = TFRMSProp(self.net.actor_params(), lr_a)
            self.opt_c = TFRMSProp(self.net.critic_params(), lr_c)
        order = getattr(self.net, "PARAM_ORDER", PARAM_ORDER)
        n_actor = getattr(self.net, "N_ACTOR_PARAMS", N_ACTOR_PARAMS)
        for opt, keys in ((self.opt_a, order[:n_actor]), (self.opt_c, order[n_actor:])):
            if adam:
                opt.m = [self._flat_view(self.flat.m, k) for k in keys]
                opt.v = [self._flat_view(self.flat.v, k) for k in keys]
            else:
                opt.ms = [self._ms_view(k) for k in keys]
        # the clip's sums of squares (actor, critic) stay on the device between the reduction and the step; read back with the loss
        self._sumsq = self._sumsq_ws = None
        if self.max_grad_norm is not None and self.dev.type == "cuda":
            from . import _agent_capi as _A

            self._sumsq = torch.zeros(2, dtype=torch.float64, device=self.dev)
            self._sumsq_ws = _A.sumsq_workspace(self.flat.n_flat, self.dev)
        self.T, self.gamma, self.beta = int(rollout), float(gamma), float(beta)
        self.update_chunk = int(update_chunk)
        self.gen = torch.Generator(device=self.dev).manual_seed(int(seed) + 1000 * int(env.env_id_base + 1))
        if first_state not in ("obs", "zeros"):
            raise ValueError("first_state must be 'obs' or 'zeros'")
        N, T, K = env.n_envs, self.T, env.nBS + env.nUE
        # rollout buffers (persistent: the captured graph holds their addresses).  idx_buf[t] = observation BEFORE step t,
        # idx_buf[T] = the state the rollout ended in (bootstrap value; copied to slot 0 when the next rollout starts).
        self.idx_buf = torch.empty((T + 1, N, K), dtype=torch.int64, device=self.dev)
        self.act_buf = torch.empty((T, N), dtype=torch.int64, device=self.dev)
        self.rew_buf = torch.empty((T, N), dtype=torch.float32, device=self.dev)
        self.u_buf = torch.empty((T, N), dtype=torch.float32, device=self.dev)
        # first_state: "obs" = the observation the constructor's channel update produced; "zeros" = what the reference's first
        # work() call sees, the all-zero env.state of a never-reset env (a2c_single_thread.py:143,155): no non-zero cell, i.e.
        # every index is -1 = "no row" and the first layer returns its bias.
        self.idx_buf[T] = obs_to_indices(env.observation(), self.G, self.B)
        if first_state == "zeros":
            self.idx_buf[T].fill_(-1)
        self.ep_r = torch.zeros(N, device=self.dev)
        self.running_r = None                                          # GLOBAL_RUNNING_R EMA, :169-172
        self.last_episode_return = None
        # A reward spec that terminates (with_collision(.., terminate=True)): envs end and restart INSIDE the rollout (_after_step), each at
        # its own step.  done_buf[t] = the done row of step t; the update's targets are cut there (nstep_returns_done, gae_done_reference).
        # _reset_mask is the mask the per-step env.reset reads (persistent: a captured graph holds its address); _fin_sum / _fin_cnt are the
        # per-env totals of the episodes that ended since _end_rollout last read them.  Without such a spec none of this exists.
        self.done_buf = None
        self.episodes_ended = None
        if getattr(self.reward_spec, "terminate", False):
            self.done_buf = torch.zeros((T, N), dtype=torch.uint8, device=self.dev)
            self._reset_mask = torch.zeros(N, dtype=torch.uint8, device=self.dev)
            self._fin_sum = torch.zeros(N, dtype=torch.float64, device=self.dev)
            self._fin_cnt = torch.zeros(N, dtype=torch.int32, device=self.dev)
        self.stats = {}
        self._tuning_frozen = False
        self._fwd_valid = False
        self._ppo = None              # while ppo_update's epochs run: adv / ret / logp_old of the batch and the clip; the loss hooks answer with the PPO form
        self._mb = None               # ppo_update with minibatches, fused: the permuted copy of the batch (_minibatch_buffers)

    def _flat_view(self, buf, key):
        p = getattr(self.net, key)
        off = (p.data_ptr() - self.flat.w.data_ptr()) // self.flat.w.element_size()
        return buf[off:off + p.numel()].view_as(p)

    def _ms_view(self, key):
        return self._flat_view(self.flat.ms, key)

    @property
    def idx(self):
        """Indices of the current observation [N, B + U] (what the next action will be chosen from)."""
        return self.idx_buf[self.T]

    # ---- rollout ---------------------------------------------------------------------------------------------------
    def _indices_into(self, out):
        if self.dev.type == "cuda":
            from . import _agent_capi as A

            A.obs_indices(self.env.observation(), self.G, self.B, out=out)
        else:
            out.copy_(obs_to_indices(self.env.observation(), self.G, self.B))

    def _first_layer(self, t, lo, hi):
        """Both trunks' first layers (relu6) for the rows [lo, hi) of step t (GPU): gathered from idx_buf[t] at t = 0 or without fused_obs,
        else with the index list built from the observation step t - 1 left behind, inside the gather (and stored to idx_buf[t])."""
        from . import _agent_capi as A

        net, fw = self.net, self._fwd
        if t == 0 or not self.fused_obs:
            # both trunks in one gather (tried twice, round 2 and round 3: the critic's half on a second stream beside the actor's GEMMs is
            # SLOWER, 6.3-6.4 against 5.5 ms per rollout: two 800-byte gathers cost more than one of 1600)
            self._gather_kernels()[0](self.idx_buf[t][lo:hi], net.a_w1, net.a_b1, net.c_w1, net.c_b1, relu6=True, out_a=fw["h1a"][t][lo:hi],
                                      out_c=fw["h1c"][t][lo:hi])
        else:
            self._gather_kernels()[1]({k: v[lo:hi] for k, v in self.env.observation().items()}, self.G, net.a_w1, net.a_b1, net.c_w1, net.c_b1,
                                      fw["h1a"][t][lo:hi], fw["h1c"][t][lo:hi], idx_out=self.idx_buf[t][lo:hi])

    # ---- what depends on the form of the policy head and on the number of nodes (factored.FactoredA2CRunner states its own) ----------
    def _gather_kernels(self):
        """(index-list gather, gather from the observation, table-gradient sort, table-gradient sums) of the first layer."""
        from . import _agent_capi as A

        return A.sparse_rows_sum, A.first_layer_from_obs, A.rows_grad_sort, A.rows_grad_sums

    def _draw(self, logits, t, lo, hi):
        """Actions of the rows [lo, hi) of step t from their logits (GPU), into act_buf[t]."""
        from . import _agent_capi as A

        A.sample_actions(logits, self.u_buf[t][lo:hi], out=self.act_buf[t][lo:hi])

    def _draw_reference(self, t):
        """Step t's actions on the CPU path: the plain PyTorch forward and draw."""
        return sample_actions(self.net.actor_only(self.idx_buf[t]), uniforms=self.u_buf[t])

    def _loss_workspace(self):
        from . import _agent_capi as A

        return A.loss_grad_workspace(self.net.n_action, self.dev)

    def _loss_grad(self, logits, v, target, actions, dv, dbias, loss, ws):
        from . import _agent_capi as A

        if self._ppo is not None:      # ``target`` (the n-step returns update_fused computed) is not used: the batch's GAE returns take its place
            s, b = self._ppo, self._upd
            if "ws_ppo" not in b:
                b["ws_ppo"] = A.ppo_loss_grad_joint_workspace(self.net.n_action, self.dev)
            A.ppo_loss_grad(logits, v, s["ret"], s["adv"], s["logp_old"], actions, self.beta, s["clip"], dv, dbias, loss, b["ws_ppo"])
        else:
            A.a2c_loss_grad(logits, v, target, actions, self.beta, dv, dbias, loss, ws)

    def _policy(self, t, lo, hi):
        """The actor's layer 2, policy head and action draw for the rows [lo, hi) of step t (GPU)."""
        from . import _agent_capi as A

        net, fw, wt = self.net, self._fwd, self._wt
        h1a, h2a, logits = fw["h1a"][t][lo:hi], fw["h2a"][t][lo:hi], fw["logits"][t][lo:hi]
        if self.fused_head:      # one launch, 32 rows per workgroup
            A.actor_head(h1a, wt["a_w2t"], net.a_b2, wt["a_w3t"], wt["a_b3p"], self.u_buf[t][lo:hi], net.n_action, h2a, self._logits_pad[t][lo:hi],
                         self.act_buf[t][lo:hi])
        elif wt is not None:     # float32 MFMA kernels, bias / relu6 fused, 64-row workgroups (8192 rows fill the chip)
            A.gemm_rows(h1a, wt["a_w2t"], h2a, w_transposed=True, bias=net.a_b2, relu6=True)
            A.gemm_rows(h2a, wt["a_w3t"], self._logits_pad[t][lo:hi], w_transposed=True, bias=wt["a_b3p"])
            self._draw(logits, t, lo, hi)
        else:
            torch.addmm(net.a_b2, h1a, net.a_w2, out=h2a).clamp_(0.0, 6.0)
            torch.addmm(net.a_b3, h2a, net.a_w3, out=logits)
            self._draw(logits, t, lo, hi)

    def _rollout_steps(self):
        """The T-step loop: choose_action (main.py:165-169) -> env.step -> next observation.  No host synchronisation, no
        allocation visible to the caller: capturable."""
        if self._persistent:
            return self._rollout_steps_persistent()
        if self._halves is not None:
            return self._rollout_steps_pipelined()
        env, T, N = self.env, self.T, self.env.n_envs
        self.idx_buf[0].copy_(self.idx_buf[T])
        cuda = self.dev.type == "cuda"
        for t in range(T):
            if cuda:
                self._first_layer(t, 0, N)
                self._policy(t, 0, N)
            else:
                self.act_buf[t] = self._draw_reference(t)
            env.step(self.act_buf[t], reward_out=self.rew_buf[t])
            self._after_step(t, cuda and self.fused_obs)

    def _after_step(self, t, fused_next=False, lo=0, hi=None):
        """The tail of rollout step t, behind env.step(.., reward_out=rew_buf[t]): stated once for every per-step loop (_rollout_steps and its
        pipelined form, FactoredA2CRunner._imitate_collect, CnnA2CRunner.collect).
        With a reward spec that terminates: the step's episode bookkeeping (uavagent_episode_step_f32: ep_r, done_buf[t], the reset mask, the
        totals of the episodes that ended), then the masked reset of the envs that ended -- unconditionally, no host synchronisation: a
        mask of zeros resets nothing -- and only then the next observation, so that idx_buf[t + 1], or the fused first layer of step t + 1
        (which reads the env's observation itself), sees the first state of the new episode.
        Then the index list of the next observation: not with ``fused_next`` (step t + 1's first layer builds it, fused_obs) unless t is the
        last step.  ``lo`` / ``hi``: the rows of one half of the pipelined form (never with a terminating spec)."""
        if self.done_buf is not None:
            self._episode_step(t)
            self.env.reset(mask=self._reset_mask)
        if fused_next and t != self.T - 1:
            return
        if hi is None:
            self._indices_into(self.idx_buf[t + 1])
        else:
            from . import _agent_capi as A

            A.obs_indices({k: v[lo:hi] for k, v in self.env.observation().items()}, self.G, self.B, out=self.idx_buf[t + 1][lo:hi])

    def _episode_step(self, t):
        """Step t's episode bookkeeping from rew_buf[t] and the done the step returned, in place (one launch on the GPU)."""
        args = (self.rew_buf[t], self.env.out["done"], self.ep_r, self.done_buf[t], self._reset_mask, self._fin_sum, self._fin_cnt)
        if self.dev.type == "cuda":
            from . import _agent_capi as A

            A.episode_step(*args)
        else:
            episode_step_reference(*args)

    def _rollout_steps_persistent(self):
        """The T-step loop as two persistent launches (see persistent_rollout in __init__): the first layer of the state the rollout starts
        from, the gates, then the policy kernel on the calling stream and the env kernel on a side stream.  Capturable."""
        from . import _agent_capi as A

        env, T, net, fw, wt = self.env, self.T, self.net, self._fwd, self._wt
        env.copy_state_to(self._persist_state)       # one 11 MB device copy per rollout: what collect() falls back on if a kernel gives up
        self.idx_buf[0].copy_(self.idx_buf[T])
        self._first_layer(0, 0, env.n_envs)
        self._gate_obs.fill_(1)
        self._gate_act.zero_()
        self._gate_claim.zero_()
        main = torch.cuda.current_stream(self.dev)
        if self._persist_stream is None:
            # a stream of its own, HIGH priority: the runtime keeps separate hardware queues per priority level, so this stream cannot land on
            # the queue of the (normal-priority) stream the policy kernel is launched on -- two kernels that wait for each other must never sit
            # behind one another in ONE queue (that ends in the bounded waits' error code, and in the fallback of _prove_persistent)
            self._persist_stream = torch.cuda.Stream(device=self.dev, priority=-1)
        side = main if self._persist_same_stream else self._persist_stream
        fork = torch.cuda.Event()
        fork.record(main)
        side.wait_event(fork)
        A.actor_head_gated(fw["h1a"], wt["a_w2t"], net.a_b2, wt["a_w3t"], wt["a_b3p"], self.u_buf, net.n_action, fw["h2a"], self._logits_pad, self.act_buf,
                           self._gate_obs, self._gate_act, self._gate_claim[1:2], spin_us=self._gate_spin_us)
        with torch.cuda.stream(side):
            env.rollout_gated(self.act_buf, self._gate_act, self._gate_obs, self._gate_claim[0:1], net.a_w1, net.a_b1, fw["h1a"], net.c_w1, net.c_b1, fw["h1c"],
                              idx_out=self.idx_buf, reward_out=self.rew_buf)
        join = torch.cuda.Event()
        join.record(side)
        main.wait_event(join)

    def _prove_persistent(self):
        """Eager launches: one trial rollout on a snapshot of the env state shows whether the two persistent kernels run side by side on the
        streams this runner uses (the stream -> hardware-queue mapping is fixed when a stream is created); if not, the per-step launches take
        over for good.  (The captured form has the same trial in _capture.)"""
        self._trial("eager trial", self._rollout_steps)
        self._persistent_proven = True

    def _trial(self, what, run):
        """Runs ``run`` (a rollout: the eager launches or the replay of their captured graph) on what a rollout changes -- the env state,
        env.out and idx_buf[T] -- synchronises and puts all three back.  Persistent form: returns whether its two kernels ran side by side;
        they did not when an entry point refused the launch or a gated wait timed out, and then the per-step launches take over for good."""
        env, T = self.env, self.T
        state = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=self.dev)
        env.copy_state_to(state)
        keep_out = {k: v.clone() for k, v in env.out.items()}
        keep_idx = self.idx_buf[T].clone()
        # (a terminating spec: the steps also keep the episode bookkeeping)
        keep_ep = [(v, v.clone()) for v in ((self.ep_r, self._fin_sum, self._fin_cnt) if self.done_buf is not None else ())]
        why = None
        try:
            run()
        except Exception as ex:                        # (persistent form: an entry point refused the shapes before launching anything)
            if not self._persistent:
                raise
            why = "refused: %s" % ex
        finally:
            torch.cuda.synchronize(self.dev)
            if why is None and self._persistent and self._persistent_failed():
                why = "a gate wait timed out"
            env.copy_state_from(state)                 # (also clears the env handle's device-error word)
            for k, v in keep_out.items():
                env.out[k].copy_(v)
            self.idx_buf[T].copy_(keep_idx)
            for v, kept in keep_ep:
                v.copy_(kept)
        if why is not None:
            self._give_up_persistent("A2CRunner: the persistent rollout kernels did not run side by side (%s: %s); using the per-step launches "
                                     "instead" % (what, why))
        return why is None

    def _give_up_persistent(self, message):
        """The persistent rollout is abandoned (warning ``message``): the per-step launches take over for good.  Clears the policy
        library's error word; the caller's restore of the env state clears the env handle's."""
        import warnings
        from . import _agent_capi as A

        warnings.warn(message)
        self._persistent = False
        A.device_error_clear()

    def _persistent_failed(self):
        """True when a gated launch gave up on the device (both libraries keep a sticky word in host-mapped memory)."""
        from . import _agent_capi as A

        return A.device_error() != 0 or self.env.device_error() != 0

    def _rollout_steps_pipelined(self):
        """The T-step loop with the batch cut in two halves, one stream each (see pipeline_halves in __init__).  Per half and step: first
        layer from the observation the half's previous step left (gather), actor head, env step of the half's envs
        (uavenv_step_range).  The heads alternate: head(half 1, t) after head(half 0, t), head(half 0, t + 1) after head(half 1, t); everything
        else overlaps them.  Capturable: the second stream forks from and joins the calling stream through events."""
        env, T = self.env, self.T
        self.idx_buf[0].copy_(self.idx_buf[T])
        main = torch.cuda.current_stream(self.dev)
        if self._pipe_stream is None:
            # (normal priority.  A high-priority stream would have a hardware queue of its own -- with a dozen streams alive in one process the
            #  side stream can end up in the calling stream's queue, where the halves run one after the other: 8.8-10.3 instead of 4.4 ms in a
            #  five-runner A/B process, profiles/r04fd_ab_collect_five_runners_in_one_process.json -- but the captured graph then runs the rollout in
            #  12.9 ms: profiles/r04gu_ab_bench_a2c_pipelined_on_a_high_priority_stream.txt)
            self._pipe_stream = torch.cuda.Stream(device=self.dev)
        side = self._pipe_stream
        fork = torch.cuda.Event()
        fork.record(main)
        side.wait_event(fork)
        last_head = None                                              # event behind the head issued last
        for t in range(T):
            for (lo, hi), st in zip(self._halves, (main, side)):
                with torch.cuda.stream(st):
                    self._first_layer(t, lo, hi)
                    if last_head is not None:
                        st.wait_event(last_head)                     # the heads run one after the other; everything else overlaps them
                    self._policy(t, lo, hi)
                    last_head = torch.cuda.Event()
                    last_head.record(st)
                    env.step_range(self.act_buf[t], lo, hi - lo, reward_out=self.rew_buf[t])
                    self._after_step(t, True, lo, hi)
        join = torch.cuda.Event()
        join.record(side)
        main.wait_event(join)

    @torch.no_grad()
    def collect(self):
        """One rollout: returns (idx [T,N,K], actions [T,N], rewards [T,N], bootstrap [N]) -- views of persistent buffers, valid
        until the next collect()."""
        env, T = self.env, self.T
        self._check_reward_spec()
        self.u_buf.copy_(torch.rand(self.u_buf.shape, device=self.dev, dtype=torch.float32, generator=self.gen))
        self._refresh_transposed()
        if self.collect_launch == "graph" and self.dev.type == "cuda" and self._graph is None:
            try:
                self._capture()
            except Exception as ex:      # a failed capture executes nothing (the warm-up pass has been rolled back): run eagerly
                import warnings

                warnings.warn("A2CRunner: hipGraph capture of the rollout failed (%s: %s); collecting eagerly" % (type(ex).__name__, ex))
                self.collect_launch = "eager"
                self._graph = None
        persistent_ran = self._persistent
        if self.collect_launch == "graph" and self._graph is not None:
            self._graph.replay()
        else:
            if self._persistent and not self._persistent_proven:
                self._prove_persistent()
                persistent_ran = self._persistent
            self._rollout_steps()
        done = env.out["done"].bool()
        any_done = bool(done.any())                                                  # (host sync: the rollout's kernels have finished)
        if persistent_ran and self._persistent_failed():
            # A persistent rollout kernel gave up waiting for its partner in the MIDDLE of a run (they had been proven to run side by side: so
            # something else kept one of them off the chip for longer than the spin budget).  Nothing is lost: the rollout started from the
            # state snapshot _rollout_steps_persistent took, the uniforms are still in u_buf -- restore, switch to the per-step launches for
            # good, and collect this rollout again: same results as if the persistent kernels had finished.
            from . import _agent_capi as A

            self._give_up_persistent("A2CRunner.collect: a persistent rollout kernel gave up waiting for its partner (device error words: policy "
                                     "0x%08x, env 0x%08x); the rollout is collected again with the per-step launches, which this runner uses from "
                                     "now on" % (A.device_error(), env.device_error()))
            env.copy_state_from(self._persist_state)                                 # (also clears the env handle's device-error word)
            self.idx_buf[T].copy_(self.idx_buf[0])
            self._graph = None                                                       # (the next collect() captures the per-step form)
            self._rollout_steps()
            done = env.out["done"].bool()
            any_done = bool(done.any())
        self._fwd_valid = self._fwd is not None
        return self._end_rollout(done, any_done)

    def _check_reward_spec(self):
        """Raises if the env's reward spec is not the one this runner was built with (see ``reward_spec`` in _init_common)."""
        now = getattr(self.env, "reward", None)
        if now != self.reward_spec:
            raise RuntimeError("%s: the env's reward is now %r, this runner was built with %r (its rollout form and captured graph hold the "
                               "old one); build a new runner after set_reward()" % (type(self).__name__, now, self.reward_spec))

    def _end_rollout(self, done, any_done):
        """After the T steps: episode returns, the bootstrap value v(s_T) (0 where done), the masked reset of the finished envs.
        -> (idx [T,N,K], actions [T,N], rewards [T,N], bootstrap [N]), views of persistent buffers valid until the next collect()."""
        env, T = self.env, self.T
        if self.done_buf is not None:
            return self._end_rollout_episodes()
        self.ep_r += self.rew_buf.sum(dim=0)
        boot = self.net.critic_only(self.idx_buf[T]).squeeze(1)                      # :173-176
        boot = torch.where(done, torch.zeros_like(boot), boot)                       # value_estimate = 0 when done
        if any_done:                                                                 # :167-172 reset_worker
            m = float(self.ep_r[done].mean())
            self.last_episode_return = m                                             # mean return of the episodes that just ended
            self.running_r = m if self.running_r is None else 0.99 * self.running_r + 0.01 * m
            self.ep_r[done] = 0.0
            env.reset(mask=done)
            self._indices_into(self.idx_buf[T])
        return self.idx_buf[:T], self.act_buf, self.rew_buf, boot

    def _end_rollout_episodes(self):
        """_end_rollout with a reward spec that terminates: the steps have kept ep_r, reset the envs that ended (a collision, or MAXSTEP --
        step_n differs from env to env now, so that end arrives mid-rollout too) and written idx_buf[T] behind the last reset.  Left: the
        bootstrap, 0 where the LAST step ended its episode (idx_buf[T] is then the next episode's first state), and the statistics of the
        episodes that ended in this rollout from the per-env totals -- their mean return, the EMA once per rollout as ever, their count."""
        T = self.T
        boot = self.net.critic_only(self.idx_buf[T]).squeeze(1)
        boot = torch.where(self.done_buf[T - 1] != 0, torch.zeros_like(boot), boot)
        n = int(self._fin_cnt.sum())                                                 # (host sync)
        self.episodes_ended = n
        if n:
            m = float(self._fin_sum.sum()) / n
            self.last_episode_return = m
            self.running_r = m if self.running_r is None else 0.99 * self.running_r + 0.01 * m
            self._fin_sum.zero_()
            self._fin_cnt.zero_()
        return self.idx_buf[:T], self.act_buf, self.rew_buf, boot

    def _batch_done(self, rew_buf):
        """The done rows of the batch ``rew_buf`` belongs to -- the runner's done_buf when it holds one of that batch's shape -- or None:
        update() keeps its signature, the done rows travel on the runner.  (A [1, m] minibatch view of ppo_update is no such batch: its
        targets were cut when the whole batch's advantages were computed.)"""
        d = self.done_buf
        return d if d is not None and tuple(rew_buf.shape) == tuple(d.shape) else None

    def _nstep_targets(self, rew_buf, boot, fused, out=None):
        """The n-step value targets [T, N] of a batch for update_fused (``fused``: the kernel) / update_reference (the PyTorch statement):
        cut at the batch's done rows when the runner holds them (_batch_done), else the plain recursion as ever."""
        done = self._batch_done(rew_buf)
        if fused:
            from . import _agent_capi as A

            if done is None:
                return A.nstep_returns(rew_buf.contiguous(), boot.contiguous(), self.gamma, out=out)
            return A.nstep_returns_done(rew_buf.contiguous(), done, boot.contiguous(), self.gamma, out=out)
        if done is None:
            return nstep_returns(rew_buf, boot, self.gamma)
        return nstep_returns_done(rew_buf, done, boot, self.gamma)

    def _refresh_transposed(self):
        """The transposed / padded copies of the actor's dense layers the rollout's GEMM kernel reads (three small copies; the captured
        graph reads the same buffers)."""
        wt = getattr(self, "_wt", None)
        if wt is not None:
            net = self.net
            wt["a_w2t"].copy_(net.a_w2.t())
            wt["c_w2t"].copy_(net.c_w2.t())
            wt["a_w3t"][:net.n_action].copy_(net.a_w3.t())
            wt["a_b3p"][:net.n_action].copy_(net.a_b3)

    def _capture(self):
        """hipGraph of the rollout loop.  A warm-up pass on a side stream first (rocBLAS handles / workspaces) and, for the persistent form,
        one trial replay of the graph, both through _trial: capturing changes nothing the caller can observe.  If either trial shows the
        persistent kernels not side by side, the per-step launches are captured instead."""
        s = torch.cuda.Stream(device=self.dev)

        def warm_up():
            s.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(s):
                self._rollout_steps()
            torch.cuda.current_stream(self.dev).wait_stream(s)

        for _ in range(2):                                # (a failed trial switches to the per-step launches, which have no trial to fail)
            if not self._trial("eager warm-up pass", warm_up):
                continue
            # capture_error_mode="thread_local": with torch.distributed initialised, RCCL's watchdog thread polls events while this
            # thread captures; in the default "global" mode that invalidates the capture.
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._rollout_steps()
            if self._persistent:
                # a graph's parallel branches need not run at the same time; the two persistent kernels must: one trial replay
                if not self._trial("trial replay of the captured graph", g.replay):
                    continue
                self._persistent_proven = True
            self._graph = g
            return

    # ---- update ----------------------------------------------------------------------------------------------------
    def update(self, idx_buf, act_buf, rew_buf, boot):
        """One gradient step on all T*N samples (a2c_single_thread.py:120-133)."""
        if self.fused_update and self.dev.type == "cuda":
            return self.update_fused(idx_buf, act_buf, rew_buf, boot)
        return self.update_reference(idx_buf, act_buf, rew_buf, boot)

    def _exchanging(self):
        """True when an update ends in a collective: more than one rank, or force_exchange with an initialised process group."""
        import torch.distributed as dist

        return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or self.force_exchange)

    def _allreduce_bucket(self, lo, hi, async_op=False):
        """Sum of flat.g[lo:hi] over ranks, in place.  nccl (RCCL): returns the work handle when async_op; gloo with CUDA tensors (the
        one-GPU rehearsal: several ranks share the card, RCCL refuses that): through the host, synchronously."""
        import torch.distributed as dist

        buf = self.flat.g[lo:hi]
        if buf.is_cuda and dist.get_backend() == "gloo":
            host = buf.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            buf.copy_(host)
            return None
        return dist.all_reduce(buf, op=dist.ReduceOp.SUM, async_op=async_op)

    def _allreduce(self, hi=None):
        """Sum of flat.g[:hi] over ranks (default: the whole flat gradient, ONE all-reduce -- RCCL over xGMI with backend nccl -- straight on
        the buffer the backward pass wrote).  -> the 1 / world_size the optimiser step folds in; 1.0 when the update ends in no collective."""
        import torch.distributed as dist

        if not self._exchanging():
            return 1.0
        self._allreduce_bucket(0, self.flat.n_flat if hi is None else hi)
        return 1.0 / dist.get_world_size()

    def _ensure_update_buffers(self, M, K):
        from . import _agent_capi as A

        # One set per row count, the two last used kept: the rollout's own M rows and a PPO minibatch's m live side by side (``_upd`` is the
        # set in use: the loss hooks read it)
        sets = self._upd_sets
        if M in sets:
            self._upd = sets[M] = sets.pop(M)                  # (re-inserted: the dict's order is the order of use)
            return self._upd
        while len(sets) >= 2:
            sets.pop(next(iter(sets)))
        H, NA, dev = HIDDEN, self.net.n_action, self.dev
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        own = self._fwd is not None and M == self.T * self.env.n_envs      # the rollout's own buffers double as the update's
        ldl = (NA + 15) // 16 * 16
        if own:
            fw = {k: self._fwd[k].view(M, H) for k in ("h1a", "h1c", "h2a")}
            logits_pad = self._logits_pad.view(M, ldl)
        else:
            fw = {"h1a": f(M, H), "h1c": f(M, H), "h2a": f(M, H)}
            logits_pad = torch.zeros((M, ldl), dtype=torch.float32, device=dev)
        self._upd = {"M": M, "own": own, "h1a": fw["h1a"], "h1c": fw["h1c"], "h2a": fw["h2a"], "logits": logits_pad[:, :NA],
                     "logits_pad": logits_pad, "h2c": f(M, H), "dh": f(M, H),
                     "gcat": f(M, 2 * H), "v": f(M), "dv": f(M), "target": f(M),
                     "loss": torch.zeros(5, dtype=torch.float64, device=dev),      # the A2C kernel writes three sums, the PPO kernel five
                    
                     "ws_loss": self._loss_workspace(), "ws_relu": A.relu6_bwd_workspace(H, dev),
                     "ws_rows": A.rows_grad_workspace(M, K, 2 * H, self.net.n_state, dev)}
        if self.hip_gemms:
            self._upd.update({"w3p": torch.zeros((H, ldl), dtype=torch.float32, device=dev),       # a_w3 in rows of ldl, zero tail
                              "ws_tn_h": A.gemm_tn_workspace(M, H, dev), "ws_tn_a": A.gemm_tn_workspace(M, NA, dev),
                              "ws_cs": A.gemm_rows_workspace(M, dev)})
            if self._exchanging() and self.overlap_allreduce:    # one table gradient per trunk: each needs its g rows contiguous
                self._upd.update({"g_a": f(M, H), "g_c": f(M, H)})
        sets[M] = self._upd
        return self._upd

    def _actor_backward(self, b, g):
        """The actor trunk backwards from d logits (in b["logits"]): dW3; dh2a = relu6'(h2a) * (dlogits @ W3^T); dW2 + db2;
        g = relu6'(h1a) * (dh2a @ W2^T), the rows the first-layer table gradient sums, + db1."""
        from . import _agent_capi as A

        net, gv, H = self.net, self.flat.gv, HIDDEN
        if self.hip_gemms:
            b["w3p"][:, :net.n_action].copy_(net.a_w3)
            A.gemm_tn(b["h2a"], b["logits"], gv["a_w3"], b["ws_tn_a"])
            A.gemm_rows(b["logits_pad"], b["w3p"], b["dh"], w_transposed=True, relu6_mask_h=b["h2a"])
            A.gemm_tn(b["h1a"], b["dh"], gv["a_w2"], b["ws_tn_h"], dbias_out=gv["a_b2"])
            A.gemm_rows(b["dh"], net.a_w2, g, w_transposed=True, relu6_mask_h=b["h1a"], colsum_out=gv["a_b1"], workspace=b["ws_cs"])
        else:
            torch.mm(b["h2a"].t(), b["logits"], out=gv["a_w3"])
            torch.mm(b["logits"], net.a_w3.t(), out=b["dh"])
            A.relu6_bwd(b["dh"], b["h2a"], b["dh"], H, gv["a_b2"], b["ws_relu"])
            torch.mm(b["h1a"].t(), b["dh"], out=gv["a_w2"])
            torch.mm(b["dh"], net.a_w2.t(), out=b["h2a"])                 # h2a is free now: reuse it for d h1a
            A.relu6_bwd(b["h2a"], b["h1a"], g, g.stride(0), gv["a_b1"], b["ws_relu"])

    def _critic_backward(self, b, g):
        """The critic trunk backwards from dv (in b["dv"]): the value head's outer product + relu6' + db2 + dw3 in one streaming kernel;
        dW2; g = relu6'(h1c) * (dh2c @ W2^T), the rows the first-layer table gradient sums, + db1."""
        from . import _agent_capi as A

        net, gv, H = self.net, self.flat.gv, HIDDEN
        A.relu6_bwd(None, b["h2c"], b["dh"], H, gv["c_b2"], b["ws_relu"], dv=b["dv"], w3=net.c_w3, dw3_out=gv["c_w3"])
        if self.hip_gemms:
            A.gemm_tn(b["h1c"], b["dh"], gv["c_w2"], b["ws_tn_h"])
            A.gemm_rows(b["dh"], net.c_w2, g, w_transposed=True, relu6_mask_h=b["h1c"], colsum_out=gv["c_b1"], workspace=b["ws_cs"])
        else:
            torch.mm(b["h1c"].t(), b["dh"], out=gv["c_w2"])
            torch.mm(b["dh"], net.c_w2.t(), out=b["h2c"])
            A.relu6_bwd(b["h2c"], b["h1c"], g, g.stride(0), gv["c_b1"], b["ws_relu"])

    @torch.no_grad()
    def update_fused(self, idx_buf, act_buf, rew_buf, boot):
        """The update with a hand-derived backward pass (same mathematics as update_reference, main.py:64-74,143-156).  Dense layers:
        libuavagent's float32 MFMA GEMMs (hip_gemms, the default: relu6 backward fused into the dX kernels' epilogue, bias gradients
        taken from the dW kernels' ones column / the dX kernels' column sums) or torch GEMMs + separate relu6-backward passes;
        softmax / loss / its gradient, the value head, the table gradient and RMSProp = libuavagent kernels.  Everything writes
        straight into the flat gradient buffer."""
        from . import _agent_capi as A

        net, fl = self.net, self.flat
        T, N, K = idx_buf.shape
        M, H = T * N, HIDDEN
        b = self._ensure_update_buffers(M, K)
        target = self._nstep_targets(rew_buf, boot, True, out=b["target"].view(T, N)).reshape(M)
        idx, act = idx_buf.reshape(M, K).contiguous(), act_buf.reshape(M)
        gv = fl.gv
        hip = self.hip_gemms
        main = torch.cuda.current_stream(self.dev)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        side = self._side
        rows_sum, _, rows_sort, rows_sums = self._gather_kernels()
        # The table gradient's sort needs only idx: on the side stream, beside the forward pass and the dX chain (one sort serves both
        # trunks' sums when they are exchanged separately).
        side.wait_stream(main)
        with torch.cuda.stream(side):
            rows_sort(idx, 2 * H, net.n_state, b["ws_rows"])
        sorted_ev = torch.cuda.Event()
        sorted_ev.record(side)

        def table_grad(g, dw0, dw1):
            main.wait_event(sorted_ev)
            rows_sums((M, K), g, H, net.n_state, dw0, dw1, b["ws_rows"])
        # forward: the actor's activations and both first layers were computed by the rollout itself, with these very weights
        reuse = b["own"] and self._fwd_valid and idx_buf.data_ptr() == self.idx_buf.data_ptr()
        if not reuse:
            rows_sum(idx, net.a_w1, net.a_b1, net.c_w1, net.c_b1, relu6=True, out_a=b["h1a"], out_c=b["h1c"])
            if hip:
                self._refresh_transposed()
                A.gemm_rows(b["h1a"], self._wt["a_w2t"], b["h2a"], w_transposed=True, bias=net.a_b2, relu6=True)
                A.gemm_rows(b["h2a"], self._wt["a_w3t"], b["logits_pad"], w_transposed=True, bias=self._wt["a_b3p"])
            else:
                torch.addmm(net.a_b2, b["h1a"], net.a_w2, out=b["h2a"]).clamp_(0.0, 6.0)
                torch.addmm(net.a_b3, b["h2a"], net.a_w3, out=b["logits"])
        self._fwd_valid = False                                        # the backward pass below overwrites logits and h2a
        if hip:
            # one arithmetic whether or not the rollout's forward pass is reused: W2^T through the k-contiguous kernels (collect() /
            # the branch above refreshed the transposed copies from these very weights)
            A.gemm_rows(b["h1c"], self._wt["c_w2t"], b["h2c"], w_transposed=True, bias=net.c_b2, relu6=True)
        else:
            torch.addmm(net.c_b2, b["h1c"], net.c_w2, out=b["h2c"]).clamp_(0.0, 6.0)
        A.rowdot(b["h2c"], net.c_w3, net.c_b3, b["v"])
        # loss and its gradient w.r.t. logits / v (logits are overwritten); d a_b3, d c_b3
        self._loss_grad(b["logits"], b["v"], target, act, b["dv"], gv["a_b3"], b["loss"], b["ws_loss"])
        gv["c_b3"].copy_(b["loss"][2:3].to(torch.float32))
        two_buckets = "g_a" in b
        ae = fl.actor_end
        ev = lambda: torch.cuda.Event(enable_timing=True)
        if two_buckets:
            # ---- more than one rank: critic trunk first, its half of the gradient on the wire while the actor trunk runs ----
            self._critic_backward(b, b["g_c"])
            table_grad(b["g_c"], gv["c_w1"], None)
            ready = torch.cuda.Event()
            ready.record(main)
            e_c0, e_c1 = ev(), ev()
            with torch.cuda.stream(side):
                side.wait_event(ready)
                e_c0.record(side)
                work_c = self._allreduce_bucket(ae, fl.n_flat, async_op=True)
                if work_c is not None:
                    work_c.wait()                                  # (the SIDE stream waits; the main stream goes on with the actor)
                e_c1.record(side)
            self._actor_backward(b, b["g_a"])
            table_grad(b["g_a"], gv["a_w1"], None)
        else:
            # one rank, or one bucket: both trunks' first-layer gradient rows side by side, both tables in one sorted pass
            self._actor_backward(b, b["gcat"][:, :H])
            self._critic_backward(b, b["gcat"][:, H:])
            table_grad(b["gcat"], gv["a_w1"], gv["c_w1"])
        # synchronise and step
        ev0, ev1 = ev(), ev()
        ev0.record()
        if two_buckets:
            g_scale = self._allreduce(ae)                              # the actor's half, behind its backward pass
            main.wait_stream(side)                                     # ... and the critic's half has landed
        else:
            g_scale = self._allreduce()
        ev1.record()
        self._optimizer_step(g_scale)
        loss, clip_stats = self._read_loss(b["loss"], g_scale)        # (synchronises)
        self.stats = {"a_loss": float(loss[0]), "c_loss": float(loss[1]), "mean_reward": float(rew_buf.mean()),
                      "grad_elems": fl.n_real, "running_r": self.running_r, "allreduce_ms": ev0.elapsed_time(ev1),
                      "forward_reused": bool(reuse), "hip_gemms": bool(hip),
                      # two buckets (critic trunk, then actor trunk): the first one's time is hidden behind the actor's backward pass
                      "allreduce_overlapped_ms": e_c0.elapsed_time(e_c1) if two_buckets else None,
                      "allreduce_buckets": [4 * (fl.n_flat - ae), 4 * ae] if two_buckets else None}
        self.stats.update(clip_stats)
        return self.stats

    # ---- the optimiser step: ONE place for A2C, the PPO epochs and imitation, for every runner ------------------
    def _optimizer_step(self, g_scale):
        """The step of both networks on the flat buffers (GPU), behind the gradient exchange: per network -- the actor's slice
        [0, actor_end) and the critic's [actor_end, n_flat) are two optimisers with two learning rates -- the sum of squares of the exchanged
        gradient where max_grad_norm is set, then uavagent_adam_f32 or uavagent_rmsprop_tf1_clipped, which read that sum on the device and
        fold g_scale = 1 / world into the norm (every rank computes the same coefficient).  The defaults (rmsprop, no clip) launch exactly the
        two uavagent_rmsprop_tf1 calls of the reference's optimiser."""
        from . import _agent_capi as A

        fl, ae = self.flat, self.flat.actor_end
        if self.optimizer == "rmsprop" and self.max_grad_norm is None:
            A.rmsprop_tf1(fl.w[:ae], fl.ms[:ae], fl.g[:ae], self.lr_a, g_scale=g_scale)
            A.rmsprop_tf1(fl.w[ae:], fl.ms[ae:], fl.g[ae:], self.lr_c, g_scale=g_scale)
            return
        for i, (lo, hi, lr) in enumerate(((0, ae, self.lr_a), (ae, fl.n_flat, self.lr_c))):
            ss = None
            if self.max_grad_norm is not None:
                ss = A.sumsq(fl.g[lo:hi], self._sumsq[i:i + 1], self._sumsq_ws)
            if self.optimizer == "adam":
                A.adam(fl.w[lo:hi], fl.m[lo:hi], fl.v[lo:hi], fl.g[lo:hi], lr, self.opt_step[i] + 1, betas=self.adam_betas, eps=self.adam_eps,
                       g_scale=g_scale, sumsq=ss, max_norm=self.max_grad_norm)
            else:
                A.rmsprop_tf1_clipped(fl.w[lo:hi], fl.ms[lo:hi], fl.g[lo:hi], lr, g_scale=g_scale, sumsq=ss, max_norm=self.max_grad_norm)

    def _read_loss(self, loss_dev, g_scale):
        """(the loss sums on the host, the clip's stats): ONE .cpu() for both, the update's only synchronisation.  Also counts the steps."""
        if self.max_grad_norm is None:
            return loss_dev.cpu(), self._count_steps(None)
        both = torch.cat([loss_dev, self._sumsq]).cpu()
        norms = [float(g_scale) * math.sqrt(x) if x >= 0.0 else float("nan") for x in both[-2:].tolist()]
        return both[:-2], self._count_steps(norms)

    def _count_steps(self, norms):
        """Advances the step numbers of the networks whose step was taken; -> the stats of a clipped update ({} without max_grad_norm):
        the norms before clipping, whether each was clipped, whether a step was skipped (a norm that is not finite)."""
        if norms is None:
            self.opt_step = [s + 1 for s in self.opt_step]
            return {}
        ok = [math.isfinite(x) for x in norms]
        self.opt_step = [s + int(k) for s, k in zip(self.opt_step, ok)]
        clipped = [k and self.max_grad_norm / (x + 1e-6) < 1.0 for x, k in zip(norms, ok)]
        return {"grad_norm_a": norms[0], "grad_norm_c": norms[1], "clipped_a": bool(clipped[0]), "clipped_c": bool(clipped[1]),
                "skipped_step": not all(ok)}

    def _reference_step(self):
        """_optimizer_step's decisions with the reference forms, on flat.g as exchanged and scaled: per network the coefficient of
        clip_coefficient applied to the gradient in place, then TFRMSProp / Adam.  -> the clip's stats."""
        fl, ae = self.flat, self.flat.actor_end
        norms = [] if self.max_grad_norm is not None else None
        for i, (opt, lo, hi) in enumerate(((self.opt_a, 0, ae), (self.opt_c, ae, fl.n_flat))):
            if norms is not None:
                coef, norm = clip_coefficient(fl.g[lo:hi], self.max_grad_norm)
                norms.append(norm)
                if not math.isfinite(norm):
                    continue
                if coef < 1.0:
                    fl.g[lo:hi].mul_(coef)
            opt.step(self.opt_step[i] + 1) if self.optimizer == "adam" else opt.step()
        return self._count_steps(norms)

    def update_reference(self, idx_buf, act_buf, rew_buf, boot):
        """The same update through autograd (the form round 1 shipped), chunked to bound activation memory; gradients
        accumulate into the flat buffer, TFRMSProp steps on views of the same flat accumulators."""
        T, N, K = idx_buf.shape
        target = self._nstep_targets(rew_buf, boot, False).reshape(T * N, 1)
        idx, act = idx_buf.reshape(T * N, K), act_buf.reshape(T * N)
        M = T * N
        self.flat.zero_grad()
        a_tot = c_tot = 0.0
        for s in range(0, M, self.update_chunk):
            e = min(M, s + self.update_chunk)
            a_prob, v = self._reference_forward(idx[s:e])
            a_loss, c_loss = self._losses(a_prob, v, act[s:e], target[s:e])
            w = (e - s) / M                                   # mean over the whole batch = weighted mean of chunks
            ((a_loss + c_loss) * w).backward()                # disjoint parameter sets: same grads as two backward()s
            a_tot += float(a_loss.detach()) * w
            c_tot += float(c_loss.detach()) * w
        g_scale = self._allreduce()
        if g_scale != 1.0:
            self.flat.g.mul_(g_scale)
        clip_stats = self._reference_step()
        self.stats = {"a_loss": a_tot, "c_loss": c_tot, "mean_reward": float(rew_buf.mean()), "grad_elems": self.flat.n_real,
                      "running_r": self.running_r, "allreduce_ms": None}
        self.stats.update(clip_stats)
        return self.stats

    def _reference_forward(self, idx):
        """(a_prob, v) with autograd, for update_reference."""
        return self.net(idx)

    def _actor_prob(self, idx):
        """The policy output for the index rows ``idx`` in PyTorch (factored.FactoredA2CRunner: under its move mask)."""
        return self.net.actor_only(idx)

    def _losses(self, a_prob, v, actions, v_target):
        """(a_loss, c_loss) of a chunk, for update_reference (a runner with another policy head states its own)."""
        if self._ppo is not None:
            return self._ppo_chunk(a_prob, v, actions, ppo_losses)
        return a2c_losses(a_prob, v, actions, v_target, self.beta)

    def _ppo_chunk(self, prob, v, actions, losses):
        """_losses in PPO mode.  update_reference hands its chunks over in row order: the cursor finds the chunk's rows of the batch."""
        s = self._ppo
        n, lo = prob.shape[0], s["cursor"]
        s["cursor"] = lo + n
        adv, logp_old = s["adv"][lo:lo + n], s["logp_old"][lo:lo + n]
        with torch.no_grad():
            dl = self._logp(prob, actions, False) - logp_old
            s["n_clipped"] += float(_ppo_clipped(torch.exp(dl), adv, s["clip"]).sum())
            s["kl_sum"] += float(-dl.sum())
        return losses(prob, v, actions, adv, s["ret"][lo:lo + n], logp_old, self.beta, s["clip"])

    def _with_episodes(self, stats):
        """``stats`` of a rollout's update; with a reward spec that terminates, ``episodes_ended`` added: the episodes that ended in it."""
        if self.done_buf is not None:
            stats["episodes_ended"] = self.episodes_ended
        return stats

    def train_rollout(self):
        stats = self._with_episodes(self.update(*self.collect()))
        if self.gemm_tuning and not self._tuning_frozen:
            # every GEMM shape of a rollout + update has now run once eagerly: no timing run may start later (inside a training loop, a
            # graph capture of the host application, or with another pick in another process)
            freeze_gemm_tuning()
            self._tuning_frozen = True
        return stats

    # ---- PPO (DESIGN.md sections 22 and 23; the MLP runners, joint and factored head): GAE(lambda) advantages, then several epochs of update() in PPO mode on one rollout, full-batch or in shuffled minibatches (section 25) ----------
    @staticmethod
    def _check_ppo(epochs, clip, lam):
        if int(epochs) != epochs or int(epochs) < 1:
            raise ValueError("epochs must be an integer >= 1")
        if not 0.0 < float(clip) < 1.0:
            raise ValueError("clip must be in (0, 1)")
        if not 0.0 <= float(lam) <= 1.0:
            raise ValueError("lam must be in [0, 1]")

    PPO = True                    # cnn_agent.CnnA2CRunner: False (its update has no PPO form)

    def _require_ppo(self):
        if not self.PPO:
            raise NotImplementedError("%s: ppo_rollout / ppo_update are built for the MLP runners (A2CRunner, factored.FactoredA2CRunner)"
                                      % type(self).__name__)

    def _logp(self, x, actions, fused):
        """log pi(a | s) [M] of the actions taken: ``fused``: x = the logits on the GPU, by kernel; else x = the policy output, in PyTorch
        (factored.FactoredA2CRunner states the product policy's pair)."""
        if fused:
            from . import _agent_capi as A

            return A.logp(x, actions)
        return logp_joint(x, actions)

    def _normalize_adv(self, adv):
        """adv <- (adv - mean) / (std + 1e-8) over the batch; with more than one rank over ALL ranks' rows: one all-reduce of (sum, sum of
        squares, count) in float64."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
        a64 = adv.double()
        s = torch.stack([a64.sum(), (a64 * a64).sum(), torch.tensor(float(adv.numel()), dtype=torch.float64, device=adv.device)])
        if s.is_cuda and dist.get_backend() == "gloo":      # (as _allreduce_bucket: through the host)
            host = s.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            s = host.to(adv.device)
        else:
            dist.all_reduce(s, op=dist.ReduceOp.SUM)
        mean = s[0] / s[2]
        std = (s[1] / s[2] - mean * mean).clamp_min(0.0).sqrt()
        return ((a64 - mean) / (std + 1e-8)).to(adv.dtype)

    @staticmethod
    def _check_minibatches(M, epochs, minibatches, target_kl, rows):
        """-> minibatches as an int; ValueError for what ppo_update cannot split or stop on (before anything is touched)."""
        if isinstance(minibatches, bool) or int(minibatches) != minibatches or int(minibatches) < 1:
            raise ValueError("minibatches must be an integer >= 1")
        if M % int(minibatches):
            raise ValueError("minibatches = %d does not divide the batch of M = %d rows" % (int(minibatches), M))
        if target_kl is not None and not (math.isfinite(float(target_kl)) and float(target_kl) > 0.0):
            raise ValueError("target_kl must be finite and > 0")
        if rows is not None:
            if not torch.is_tensor(rows) or rows.dtype != torch.int64 or tuple(rows.shape) != (int(epochs), M):
                raise ValueError("rows must be an int64 [epochs, M] = [%d, %d] tensor" % (int(epochs), M))
            if not torch.equal(torch.sort(rows, dim=1).values.cpu(), torch.arange(M).expand(int(epochs), M)):
                raise ValueError("rows: every row must be a permutation of range(M = %d)" % M)
        return int(minibatches)

    def ppo_rollout(self, epochs=4, clip=0.2, lam=0.95, normalize_adv=True, minibatches=1, target_kl=None, rows=None):
        """One rollout and ``epochs`` epochs of PPO on it: GAE(lam) advantages under the critic as it stands after the rollout,
        log pi_old from the rollout's own logits, then per step the clipped surrogate (ratio clipped to 1 +- clip) with the entropy bonus for
        the actor and the squared error against the GAE returns for the critic -- update()'s forward, backward, all-reduce and optimiser
        step as they stand, with the loss hooks in PPO mode.  ``normalize_adv``: adv <- (adv - mean) / (std + 1e-8) over the batch (of all ranks).
        With epochs=1, lam=1, normalize_adv=False this is train_rollout()'s update up to float32 rounding.

        ``minibatches`` = k (it must divide M = T * N): every epoch draws a permutation of the M rows from the runner's
        generator and takes k optimiser steps, step j on rows [j * M / k, (j + 1) * M / k) of the permuted batch.  Advantages, their
        normalisation and log pi_old are the whole batch's, computed once.  ``rows``: int64 [epochs, M], the permutations to use in place of
        drawn ones (the generator is then left alone).  With k = 1 and no ``rows`` an epoch is one step on the batch as it lies, as ever.
        ``target_kl``: after every epoch, kl = the mean over its steps of the loss's mean(logp_old - logp), over all ranks; kl > target_kl
        skips the epochs that remain.  That is the k1 estimator: each step measures it BEFORE stepping, it may be negative, and with k = 1
        the first epoch's is exactly 0, so that a stop comes after the second epoch at the earliest.  Its sampling error falls with the row
        count: at production batches (51 200 to 409 600 rows) it is far below any useful target, at a few hundred rows it is not.

        Returns the last step's stats with ``clip_fraction`` and ``approx_kl`` (the last epoch's means over its steps), ``epochs`` (epochs
        run), ``minibatches``, ``early_stop`` and ``approx_kl_epochs`` (every epoch's kl, as compared with the target) added."""
        self._require_ppo()
        self._check_ppo(epochs, clip, lam)
        self._check_minibatches(self.T * self.env.n_envs, epochs, minibatches, target_kl, rows)
        return self._with_episodes(self.ppo_update(*self.collect(), epochs=epochs, clip=clip, lam=lam, normalize_adv=normalize_adv,
                                                   minibatches=minibatches, target_kl=target_kl, rows=rows))

    def _mean_over_ranks(self, x):
        """The mean of a host float over the ranks (itself with one rank), as _normalize_adv exchanges its sums."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return x
        t = torch.tensor([x], dtype=torch.float64, device="cpu" if dist.get_backend() == "gloo" else self.dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return float(t[0]) / dist.get_world_size()

    def _minibatch_buffers(self, M, K, like):
        """The permuted copy of a batch's five per-row arrays (fused path), kept from call to call: ppo_shuffle_rows writes it once per epoch."""
        mb = self._mb
        if mb is None or mb["key"] != (M, K):
            e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=like.device)
            mb = self._mb = {"key": (M, K), "out": (e((M, K), torch.int64), e((M,), torch.int64), e((M,), torch.float32),
                                                    e((M,), torch.float32), e((M,), torch.float32))}
        return mb["out"]

    @torch.no_grad()
    def _ppo_prepare(self, idx_buf, act_buf, rew_buf, boot, lam, normalize_adv, fused):
        """(adv, ret, logp_old), float32 [M], of the batch under the weights as they stand.  ``fused``: libuavagent's logp and GAE kernels on the
        rollout's own logits and critic rows (recomputed if an update has overwritten them); else the PyTorch statements."""
        T, N, K = idx_buf.shape
        M = T * N
        idx, act = idx_buf.reshape(M, K), act_buf.reshape(M)
        if fused:
            from . import _agent_capi as A

            net, b = self.net, self._ensure_update_buffers(M, K)
            if not (b["own"] and self._fwd_valid and idx_buf.data_ptr() == self.idx_buf.data_ptr()):
                rows_sum = self._gather_kernels()[0]
                rows_sum(idx.contiguous(), net.a_w1, net.a_b1, net.c_w1, net.c_b1, relu6=True, out_a=b["h1a"], out_c=b["h1c"])
                if self.hip_gemms:
                    self._refresh_transposed()
                    A.gemm_rows(b["h1a"], self._wt["a_w2t"], b["h2a"], w_transposed=True, bias=net.a_b2, relu6=True)
                    A.gemm_rows(b["h2a"], self._wt["a_w3t"], b["logits_pad"], w_transposed=True, bias=self._wt["a_b3p"])
                else:
                    torch.addmm(net.a_b2, b["h1a"], net.a_w2, out=b["h2a"]).clamp_(0.0, 6.0)
                    torch.addmm(net.a_b3, b["h2a"], net.a_w3, out=b["logits"])
                # the update's buffers now hold this batch's forward pass under the current weights: epoch 0 reuses it where they are the rollout's
                self._fwd_valid = b["own"] and idx_buf.data_ptr() == self.idx_buf.data_ptr()
            logp_old = self._logp(b["logits"], act.contiguous(), True)
            if self.hip_gemms:
                A.gemm_rows(b["h1c"], self._wt["c_w2t"], b["h2c"], w_transposed=True, bias=net.c_b2, relu6=True)
            else:
                torch.addmm(net.c_b2, b["h1c"], net.c_w2, out=b["h2c"]).clamp_(0.0, 6.0)
            A.rowdot(b["h2c"], net.c_w3, net.c_b3, b["v"])
            done = self._batch_done(rew_buf)
            if done is None:
                adv, ret = A.gae(rew_buf.contiguous(), b["v"].view(T, N), boot.contiguous(), self.gamma, lam)
            else:
                adv, ret = A.gae_done(rew_buf.contiguous(), b["v"].view(T, N), done, boot.contiguous(), self.gamma, lam)
        else:
            net, logp_old, values = self.net, [], []
            for s in range(0, M, self.update_chunk):
                e = min(M, s + self.update_chunk)
                logp_old.append(self._logp(self._actor_prob(idx[s:e]), act[s:e], False))
                values.append(net.critic_only(idx[s:e]).reshape(-1))
            logp_old = torch.cat(logp_old)
            done = self._batch_done(rew_buf)
            if done is None:
                adv, ret = gae_reference(rew_buf, torch.cat(values).view(T, N), boot, self.gamma, lam)
            else:
                adv, ret = gae_done_reference(rew_buf, torch.cat(values).view(T, N), done, boot, self.gamma, lam)
        adv, ret = adv.reshape(M), ret.reshape(M)
        if normalize_adv:
            adv = self._normalize_adv(adv)
        return adv.contiguous(), ret.contiguous(), logp_old

    def ppo_update(self, idx_buf, act_buf, rew_buf, boot, epochs=4, clip=0.2, lam=0.95, normalize_adv=True, fused=None, minibatches=1,
                   target_kl=None, rows=None):
        """ppo_rollout's update on a collected batch.  ``fused``: None = update()'s choice, True / False = the kernels and update_fused /
        the PyTorch statements and update_reference.  With minibatches (or ``rows``) the batch's five per-row arrays are permuted once per
        epoch -- fused: ONE uavagent_ppo_shuffle_rows launch; else index_select -- and step j is update_fused / update_reference on rows
        [j * m, (j + 1) * m) of the copy as a [1, m] rollout with a zero bootstrap, the loss hooks reading that slice's adv / ret / logp_old."""
        self._require_ppo()
        self._check_ppo(epochs, clip, lam)
        T, N, K = idx_buf.shape
        M = T * N
        k = self._check_minibatches(M, epochs, minibatches, target_kl, rows)
        m = M // k
        permuted = k > 1 or rows is not None      # else: an epoch is one step on the batch as it lies, the code path of the full-batch PPO
        if fused is None:
            fused = self.fused_update and self.dev.type == "cuda"
        step = self.update_fused if fused else self.update_reference
        adv, ret, logp_old = self._ppo_prepare(idx_buf, act_buf, rew_buf, boot, float(lam), bool(normalize_adv), fused)
        self._ppo = {"adv": adv, "ret": ret, "logp_old": logp_old, "clip": float(clip)}
        kls, early_stop = [], False
        try:
            if permuted:
                self._fwd_valid = False            # every step recomputes its forward pass, on its own rows
                src = (idx_buf.reshape(M, K).contiguous(), act_buf.reshape(M).contiguous(), adv, ret, logp_old)
                zero_rew, zero_boot = torch.zeros((1, m), dtype=rew_buf.dtype, device=rew_buf.device), torch.zeros(m, dtype=boot.dtype, device=boot.device)
                mean_reward = float(rew_buf.mean())
            for e in range(int(epochs)):
                if permuted:
                    perm = rows[e].to(self.dev) if rows is not None else torch.randperm(M, generator=self.gen, device=self.dev)
                    if fused:
                        from . import _agent_capi as A

                        cp = A.ppo_shuffle_rows(perm.contiguous(), *src, out=self._minibatch_buffers(M, K, src[0]))
                    else:
                        cp = tuple(t.index_select(0, perm) for t in src)
                clip_e = kl_e = 0.0
                for j in range(k):
                    if permuted:
                        lo, hi = j * m, (j + 1) * m
                        self._ppo = {"adv": cp[2][lo:hi], "ret": cp[3][lo:hi], "logp_old": cp[4][lo:hi], "clip": float(clip)}
                        args = (cp[0][lo:hi].view(1, m, K), cp[1][lo:hi].view(1, m), zero_rew, zero_boot)
                    else:
                        args = (idx_buf, act_buf, rew_buf, boot)
                    self._ppo.update(cursor=0, n_clipped=0.0, kl_sum=0.0)
                    stats = step(*args)
                    self._fwd_valid = False                                # the weights have moved: later steps recompute the forward pass
                    if fused:
                        loss = self._upd["loss"].cpu()
                        clip_j, kl_j = float(loss[3]), float(loss[4])
                    else:
                        clip_j, kl_j = self._ppo["n_clipped"] / m, self._ppo["kl_sum"] / m
                    clip_e, kl_e = clip_e + clip_j, kl_e + kl_j
                if k > 1:
                    clip_e, kl_e = clip_e / k, kl_e / k
                stats["clip_fraction"], stats["approx_kl"] = clip_e, kl_e
                if target_kl is not None:
                    kl_e = self._mean_over_ranks(kl_e)                     # every rank compares the same number: all stop in the same epoch
                kls.append(kl_e)
                if target_kl is not None and kl_e > float(target_kl) and e + 1 < int(epochs):
                    early_stop = True
                    break
            if permuted:
                stats["mean_reward"] = mean_reward                         # (the steps saw the zero rewards of their [1, m] views)
                if fused:
                    stats["forward_reused"] = False
            stats.update(epochs=len(kls), minibatches=k, early_stop=early_stop, approx_kl_epochs=kls)
        finally:
            self._ppo = None
        return stats

    # ---- checkpoint / resume (the reference saves the actor only and cannot resume) -------------------------------
    def state_dict(self):
        """Everything a bit-identical continuation needs: both trunks and their RMSProp accumulators (the flat buffers), the env batch
        (state blob + last outputs), the current observation indices, the episode bookkeeping and the action-sampling generator."""
        env = self.env
        blob = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=self.dev)
        env.copy_state_to(blob)
        sd = {"format": 1, "n_envs": env.n_envs, "n_bs": env.nBS, "n_ue": env.nUE, "grid_n": env.grid_n, "rollout": self.T,
              "w": self.flat.w.detach().cpu(), "ms": self.flat.ms.detach().cpu(), "env_state": blob.cpu(), "env_out": env._arena.cpu(),
              "idx": self.idx_buf[self.T].cpu(), "ep_r": self.ep_r.cpu(), "running_r": self.running_r,
              "last_episode_return": self.last_episode_return, "gen_state": self.gen.get_state().cpu()}
        if self.optimizer == "adam":      # (the default optimiser's dict keeps exactly the keys it had)
            sd.update({"optimizer": "adam", "opt_step": list(self.opt_step), "m": self.flat.m.detach().cpu(), "v": self.flat.v.detach().cpu()})
        return sd

    def load_state_dict(self, sd):
        env = self.env
        shape = (sd["n_envs"], sd["n_bs"], sd["n_ue"], sd["grid_n"], sd["rollout"])
        if sd.get("net", "mlp") != self.NET_KIND:
            raise ValueError("checkpoint holds a %s network, this runner trains a %s one" % (sd.get("net", "mlp"), self.NET_KIND))
        if sd.get("format") != 1 or shape != (env.n_envs, env.nBS, env.nUE, env.grid_n, self.T):
            raise ValueError("checkpoint was written for another configuration: %r" % (shape,))
        if sd.get("optimizer", "rmsprop") != self.optimizer:
            raise ValueError("checkpoint was written with optimizer %r, this runner steps with %r" % (sd.get("optimizer", "rmsprop"),
                                                                                                     self.optimizer))
        with torch.no_grad():
            self.flat.w.copy_(sd["w"])
            self.flat.ms.copy_(sd["ms"])
            if self.optimizer == "adam":
                self.flat.m.copy_(sd["m"])
                self.flat.v.copy_(sd["v"])
                self.opt_step = [int(x) for x in sd["opt_step"]]
            env.copy_state_from(sd["env_state"].to(self.dev))
            env._arena.copy_(sd["env_out"])
            self.idx_buf[self.T].copy_(sd["idx"])
            self.ep_r.copy_(sd["ep_r"])
        self.running_r, self.last_episode_return = sd["running_r"], sd["last_episode_return"]
        self.gen.set_state(sd["gen_state"].cpu())
        self._fwd_valid = False
        torch.cuda.synchronize(self.dev) if self.dev.type == "cuda" else None


ACTOR_KEYS = ("a_w1", "a_b1", "a_w2", "a_b2", "a_w3", "a_b3")   # TF order: la/kernel, la/bias, la2/kernel, la2/bias, ap/kernel, ap/bias


def save_actor_npz(net, path):
    """Actor parameters, the content of the reference's Global_A_PARA.npz (main.py:265-269: np.savez(path,
    SESS.run(a_params))).  The reference stores the ragged list as ONE pickled object array ('arr_0'); here the same
    six arrays are stored under names, so loading never needs allow_pickle."""
    import numpy as np

    np.savez(path, **{k: getattr(net, k).detach().cpu().numpy() for k in getattr(net, "ACTOR_KEYS", ACTOR_KEYS)})


def load_actor_npz(net, path):
    """Inverse of save_actor_npz (main_test.py:11-26 assigns the six arrays to the actor variables in order)."""
    import numpy as np

    keys = getattr(net, "ACTOR_KEYS", ACTOR_KEYS)
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in keys if k not in z.files]
        if missing:
            other = "CNN" if "a_conv1_k" in z.files else ("MLP" if "a_w1" in z.files else None)
            if other is not None:
                raise ValueError("%s holds a %s actor, the network is %s (train and evaluate with the same --net)" % (
                    path, other, "a CNN (CnnACNet)" if keys is not ACTOR_KEYS else "an MLP (ACNet)"))
            raise ValueError("not an actor checkpoint written by save_actor_npz (missing %s); the reference's own "
                             "Global_A_PARA.npz is a pickled object array and is not loaded" % missing)
        with torch.no_grad():
            for k in keys:
                p = getattr(net, k)
                a = torch.as_tensor(z[k])
                if tuple(a.shape) != tuple(p.shape):
                    raise ValueError("%s: checkpoint shape %s != network shape %s" % (k, tuple(a.shape), tuple(p.shape)))
                p.copy_(a.to(p.device, p.dtype))
    return net


def grad_allreduce_bytes(net):
    """Bytes of real gradient per all-reduce (the flat buffer adds < 1 KB of alignment padding)."""
    return 4 * sum(p.numel() for p in net.parameters())


def expected_param_count(n_state, n_action, hidden=HIDDEN):
    """20 206 626 parameters at G = 100, 4 UAVs (80.8 MB float32)."""
    actor = n_state * hidden + hidden + hidden * hidden + hidden + hidden * n_action + n_action
    critic = n_state * hidden + hidden + hidden * hidden + hidden + hidden + 1
    return actor + critic
