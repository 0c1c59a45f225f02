"""CNN actor-critic (the reference's netType='CNN', main.py:88-140) + synchronous A2C, on libuavcnn.so's kernels.

  network   two trunks, no shared weights:  NHWC state [N, G, G, nBS+1] (tf.reshape(s, [-1, nBS+1, G, G]) transposed; axis h = the
            cell's x, axis w = its y) -> conv 5x5 x10 relu -> conv 5x5 x10 relu -> conv 5x5 x10 relu ('valid', stride 1) -> flatten in
            (h, w, c) order, D = (G-12)^2 * 10 -> dense 100 relu6 -> {N_A softmax | 1}.  Kernels N(0, 0.1) from torch.Generator(seed),
            biases 0; parameters in TF shapes (HWIO conv kernels, [in, out] dense kernels), ten per trunk in the order of the reference's
            a_params / c_params.  The loss, the TF1 RMSProp, the n-step returns and the rollout are agent.py's.

MI355X-side design: the observation is the count map with <= nBS + nUE non-zero cells, so conv1 is a gather from the
compact index list (agent.obs_to_indices) and the dense observation is never built on the training path; conv2 / conv3 and their dX
are implicit GEMMs on float32 MFMA, the 77 440-wide dense layer is split over its reduction.  The heads reuse libuavagent.so.
``forward_reference`` (F.conv2d on the dense observation) is the reference implementation and the CPU path.
"""
import torch
import torch.nn.functional as F

from .agent import ENTROPY_BETA, GAMMA, LR_A, LR_C, A2CRunner, sample_actions

KSIZE, FILTERS, DENSE = 5, 10, 100     # main.py:93-101 (conv2d(filters=10, kernel_size=5)), :103 (dense(100, relu6))

_TRUNK = ("conv1_k", "conv1_b", "conv2_k", "conv2_b", "conv3_k", "conv3_b")
ACTOR_KEYS = tuple("a_" + k for k in _TRUNK) + ("a_la2_k", "a_la2_b", "a_ap_k", "a_ap_b")
CRITIC_KEYS = tuple("c_" + k for k in _TRUNK) + ("c_lc2_k", "c_lc2_b", "c_v_k", "c_v_b")


def flat_dim(grid_n):
    return (int(grid_n) - 3 * (KSIZE - 1)) ** 2 * FILTERS


def expected_param_count(n_bs, grid_n, n_action):
    """15 563 986 at G = 100, 4 UAVs, 625 actions (7 813 505 actor + 7 750 481 critic)."""
    convs = KSIZE * KSIZE * (n_bs + 1) * FILTERS + FILTERS + 2 * (KSIZE * KSIZE * FILTERS * FILTERS + FILTERS)
    D = flat_dim(grid_n)
    actor = convs + D * DENSE + DENSE + DENSE * n_action + n_action
    critic = convs + D * DENSE + DENSE + DENSE + 1
    return actor, critic


def dense_from_idx(idx, n_bs, grid_n, dtype=torch.float32):
    """The reference's raveled (nBS+1, G, G) count map [M, (nBS+1) G^2] from the index list; -1 (or any index out of range) adds nothing."""
    n = (int(n_bs) + 1) * int(grid_n) ** 2
    keep = ((idx >= 0) & (idx < n)).to(dtype)
    out = torch.zeros((idx.shape[0], n), dtype=dtype, device=idx.device)
    return out.scatter_add_(1, idx.clamp(0, n - 1), keep)


def conv1_from_idx_reference(idx, k1, b1, n_bs, grid_n):
    """conv1 + relu (NHWC [M, G-4, G-4, 10]) from the index list in plain PyTorch: a sum of kernel taps over the nodes, bias last (the
    arithmetic of uavcnn_conv1_from_idx_f32); equals conv1 on dense_from_idx(idx)."""
    G, C, So = int(grid_n), int(n_bs) + 1, int(grid_n) - KSIZE + 1
    M, K = idx.shape
    ok = (idx >= 0) & (idx < C * G * G)
    v = idx.clamp(min=0)
    c, x, y = v // (G * G), (v // G) % G, v % G
    acc = torch.zeros((M, So, So, FILTERS), dtype=k1.dtype, device=k1.device)
    rows = torch.arange(M, device=idx.device)
    for k in range(K):
        for i in range(KSIZE):
            for j in range(KSIZE):
                p, q = x[:, k] - i, y[:, k] - j
                sel = ok[:, k] & (p >= 0) & (p < So) & (q >= 0) & (q < So)
                if bool(sel.any()):
                    acc[rows[sel], p[sel], q[sel]] += k1[i, j, c[sel, k]]
    return F.relu(acc + b1)


class CnnACNet(torch.nn.Module):
    """Actor and critic trunks of main.py:88-140 (netType='CNN').  ``forward(idx)`` / ``actor_only`` / ``critic_only`` take the index
    list like agent.ACNet: CUDA tensors go through libuavcnn.so (+ libuavagent.so for the heads), CPU tensors through
    ``forward_reference`` on the dense observation built from idx."""

    PARAM_ORDER = ACTOR_KEYS + CRITIC_KEYS
    N_ACTOR_PARAMS = len(ACTOR_KEYS)
    ACTOR_KEYS = ACTOR_KEYS

    def __init__(self, n_bs, grid_n, n_action, seed=6):
        super().__init__()
        if not 13 <= int(grid_n) <= 200:
            raise ValueError("CnnACNet: grid_n must lie in [13, 200] (three 5x5 'valid' convolutions)")
        g = torch.Generator().manual_seed(int(seed))    # TENSOR_SEED = 6 (main.py:26), agent.ACNet's convention
        def w(*shape):
            return torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.1)   # random_normal_initializer(0, .1)
        def b(n):
            return torch.nn.Parameter(torch.zeros(n))
        self.n_bs, self.grid_n, self.n_action = int(n_bs), int(grid_n), int(n_action)
        self.n_state = (self.n_bs + 1) * self.grid_n ** 2
        C, D = self.n_bs + 1, flat_dim(grid_n)
        for pre, head in (("a", (("la2", DENSE), ("ap", self.n_action))), ("c", (("lc2", DENSE), ("v", 1)))):
            setattr(self, pre + "_conv1_k", w(KSIZE, KSIZE, C, FILTERS))
            setattr(self, pre + "_conv1_b", b(FILTERS))
            for l in (2, 3):
                setattr(self, pre + "_conv%d_k" % l, w(KSIZE, KSIZE, FILTERS, FILTERS))
                setattr(self, pre + "_conv%d_b" % l, b(FILTERS))
            (n1, w1), (n2, w2) = head
            setattr(self, "%s_%s_k" % (pre, n1), w(D, w1))
            setattr(self, "%s_%s_b" % (pre, n1), b(w1))
            setattr(self, "%s_%s_k" % (pre, n2), w(DENSE, w2))
            setattr(self, "%s_%s_b" % (pre, n2), b(w2))

    def actor_params(self):
        return [getattr(self, k) for k in ACTOR_KEYS]

    def critic_params(self):
        return [getattr(self, k) for k in CRITIC_KEYS]

    # ---- reference (plain PyTorch, autograd) ----------------------------------------------------------------------------------------
    def _trunk_reference(self, s, pre):
        M, G = s.shape[0], self.grid_n
        x = s.reshape(M, self.n_bs + 1, G, G)          # NCHW with H = x, W = y: TF's NHWC transpose of the same tensor
        for l in (1, 2, 3):
            k = getattr(self, "%s_conv%d_k" % (pre, l))
            x = F.relu(F.conv2d(x, k.permute(3, 2, 0, 1), getattr(self, "%s_conv%d_b" % (pre, l))))
        flat = x.permute(0, 2, 3, 1).reshape(M, -1)    # tf.contrib.layers.flatten of NHWC: (h, w, c) order
        n = "la2" if pre == "a" else "lc2"
        return F.relu6(flat @ getattr(self, "%s_%s_k" % (pre, n)) + getattr(self, "%s_%s_b" % (pre, n)))

    def forward_reference(self, dense_obs):
        """dense_obs float [M, (nBS+1) G^2], the raveled state as the reference feeds it -> (a_prob [M, N_A], v [M, 1])."""
        ha, hc = self._trunk_reference(dense_obs, "a"), self._trunk_reference(dense_obs, "c")
        return torch.softmax(ha @ self.a_ap_k + self.a_ap_b, dim=-1), hc @ self.c_v_k + self.c_v_b

    def _dense(self, idx):
        return dense_from_idx(idx, self.n_bs, self.grid_n, self.a_conv1_k.dtype)

    # ---- index-list entry points (agent.ACNet's signatures) ------------------------------------------------------------------------
    def forward(self, idx):
        if idx.is_cuda:
            ha, hc = _trunks_cuda(self, idx, ("a", "c"))
            return torch.softmax(_logits_cuda(self, ha), dim=-1), _value_cuda(self, hc)
        return self.forward_reference(self._dense(idx))

    def actor_only(self, idx):
        if idx.is_cuda:
            (ha,) = _trunks_cuda(self, idx, ("a",))
            return torch.softmax(_logits_cuda(self, ha), dim=-1)
        ha = self._trunk_reference(self._dense(idx), "a")
        return torch.softmax(ha @ self.a_ap_k + self.a_ap_b, dim=-1)

    def critic_only(self, idx):
        if idx.is_cuda:
            (hc,) = _trunks_cuda(self, idx, ("c",))
            return _value_cuda(self, hc)
        return self._trunk_reference(self._dense(idx), "c") @ self.c_v_k + self.c_v_b


# ---- GPU forward pieces (no autograd) ------------------------------------------------------------------------------------------------
def _act(M, S, dev):
    return torch.empty((M, S, S, FILTERS), dtype=torch.float32, device=dev)


@torch.no_grad()
def _trunk_tail(net, pre, c1, c2, c3, h, ws_dense):
    """conv2, conv3 and the dense layer of one trunk from its conv1 output (all outputs given)."""
    from . import _cnn_capi as K

    M = c1.shape[0]
    K.conv5(c1, getattr(net, pre + "_conv2_k"), c2, bias=getattr(net, pre + "_conv2_b"))
    K.conv5(c2, getattr(net, pre + "_conv3_k"), c3, bias=getattr(net, pre + "_conv3_b"))
    n = "la2" if pre == "a" else "lc2"
    K.dense_fwd(c3.view(M, -1), getattr(net, "%s_%s_k" % (pre, n)), getattr(net, "%s_%s_b" % (pre, n)), h, ws_dense)
    return h


@torch.no_grad()
def _trunks_cuda(net, idx, pres):
    """relu6 dense outputs [M, 100] of the trunks named in pres ("a", "c"), conv1 of both from one gather."""
    from . import _cnn_capi as K

    idx = idx.contiguous()
    M, G, dev = idx.shape[0], net.grid_n, idx.device
    c1 = {p: _act(M, G - 4, dev) for p in pres}
    kk = [(getattr(net, p + "_conv1_k"), getattr(net, p + "_conv1_b"), c1[p]) for p in pres]
    K.conv1_from_idx(idx, net.n_bs, G, *kk[0], *(kk[1] if len(kk) > 1 else (None, None, None)))
    ws = K.dense_fwd_workspace(M, flat_dim(G), dev)
    return [_trunk_tail(net, p, c1[p], _act(M, G - 8, dev), _act(M, G - 12, dev), torch.empty((M, DENSE), device=dev), ws) for p in pres]


def _head_copies(net, dev):
    """The policy head in the form uavagent_gemm_rows_f32 reads fastest: ap kernel transposed into rows of 640 (zero rows beyond N_A) and
    its bias padded with zeros."""
    ldl = (net.n_action + 15) // 16 * 16
    apt = torch.zeros((ldl, DENSE), dtype=torch.float32, device=dev)
    apb = torch.zeros(ldl, dtype=torch.float32, device=dev)
    apt[:net.n_action].copy_(net.a_ap_k.detach().t())
    apb[:net.n_action].copy_(net.a_ap_b.detach())
    return apt, apb


@torch.no_grad()
def _logits_cuda(net, h, apt=None, apb=None, out=None):
    from . import _agent_capi as A

    if apt is None:
        apt, apb = _head_copies(net, h.device)
    if out is None:
        out = torch.empty((h.shape[0], apt.shape[0]), dtype=torch.float32, device=h.device)
    A.gemm_rows(h, apt, out, w_transposed=True, bias=apb)
    return out[:, :net.n_action]


@torch.no_grad()
def _value_cuda(net, h, out=None):
    from . import _agent_capi as A

    if out is None:
        out = torch.empty(h.shape[0], dtype=torch.float32, device=h.device)
    A.rowdot(h, net.c_v_k.detach().reshape(-1), net.c_v_b.detach(), out)
    return out.view(-1, 1)


class CnnA2CRunner(A2CRunner):
    """Synchronous A2C with the CNN actor-critic: A2CRunner's semantics (rollout, n-step returns, loss, TF1 RMSProp, checkpoint) and its
    shared plumbing (FlatParams, episode bookkeeping, bootstrap, masked reset, update_reference, state_dict), with the CNN's own rollout
    step and hand-derived backward pass.  Launches are eager: a step is milliseconds of MFMA work.

    update_chunk: samples per forward + backward pass of the update.  Each sample holds both trunks' conv activations (2 x 1.02 MB at
    G = 100) and one trunk's backward buffers (1.02 MB): about 3.1 MB, so the default 4096 needs 12.5 GB, beside 8.3 GB of rollout
    activations at 8192 envs; an 8192 x 50 update runs in 100 chunks.  One process only: a process group of more than one rank is refused."""

    NET_KIND = "cnn"
    PPO = False                   # ppo_rollout / ppo_update raise NotImplementedError: PPO is built for the MLP runners

    def __init__(self, env, net=None, rollout=50, gamma=GAMMA, beta=ENTROPY_BETA, lr_a=LR_A, lr_c=LR_C, seed=6, update_chunk=4096,
                 first_state="obs", fused_update=True, optimizer="rmsprop", max_grad_norm=None, adam_betas=(0.9, 0.999), adam_eps=1e-8,
                 mask_margin=None):
        import torch.distributed as dist

        if mask_margin is not None:
            raise ValueError("%s: mask_margin serves the factored MLP learner (factored.FactoredA2CRunner) only" % type(self).__name__)

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("CnnA2CRunner: multi-rank CNN training is not supported (world size %d)" % dist.get_world_size())
        if net is None:
            net = CnnACNet(env.nBS, env.grid_n, env.action_space_dim, seed=seed)
        if not isinstance(net, CnnACNet):
            raise TypeError("CnnA2CRunner trains a CnnACNet")
        self._init_common(env, net, rollout, gamma, beta, lr_a, lr_c, seed, update_chunk, first_state, False, optimizer, max_grad_norm,
                          adam_betas, adam_eps)
        self.fused_update = bool(fused_update)
        self.force_exchange = False
        self._roll = None
        self._upd = None
        self._wt = None
        if self.dev.type == "cuda":
            N, G, dev = env.n_envs, self.G, self.dev
            from . import _cnn_capi as K

            self._roll = {"c1": _act(N, G - 4, dev), "c2": _act(N, G - 8, dev), "c3": _act(N, G - 12, dev),
                          "h": torch.empty((N, DENSE), device=dev), "ws": K.dense_fwd_workspace(N, flat_dim(G), dev)}
            ldl = (self.net.n_action + 15) // 16 * 16
            self._roll["logits_pad"] = torch.zeros((N, ldl), device=dev)
            f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
            self._wt = {"ap_t": torch.zeros((ldl, DENSE), device=dev), "ap_b": torch.zeros(ldl, device=dev),
                        "ap_p": torch.zeros((DENSE, ldl), device=dev)}
            for p in ("a", "c"):
                for l in (2, 3):
                    self._wt["%s_conv%d_flip" % (p, l)] = f(KSIZE, KSIZE, FILTERS, FILTERS)

    def _reference_forward(self, idx):
        return self.net.forward_reference(self.net._dense(idx))

    @torch.no_grad()
    def _refresh_transposed(self):
        """Copies the kernels read, refreshed from the parameters: the policy head transposed / padded (rollout) and in rows of 640
        (update), the conv2 / conv3 kernels flipped for dX, K'[i, j, f, c] = K[4-i, 4-j, c, f]."""
        wt, net, na = self._wt, self.net, self.net.n_action
        if wt is None:
            return
        wt["ap_t"][:na].copy_(net.a_ap_k.t())
        wt["ap_b"][:na].copy_(net.a_ap_b)
        wt["ap_p"][:, :na].copy_(net.a_ap_k)
        for p in ("a", "c"):
            for l in (2, 3):
                wt["%s_conv%d_flip" % (p, l)].copy_(getattr(net, "%s_conv%d_k" % (p, l)).flip(0, 1).permute(0, 1, 3, 2))

    def _policy_step(self, t):
        from . import _agent_capi as A
        from . import _cnn_capi as K

        net, r, N = self.net, self._roll, self.env.n_envs
        K.conv1_from_idx(self.idx_buf[t], self.B, self.G, net.a_conv1_k, net.a_conv1_b, r["c1"])
        _trunk_tail(net, "a", r["c1"], r["c2"], r["c3"], r["h"], r["ws"])
        A.gemm_rows(r["h"], self._wt["ap_t"], r["logits_pad"], w_transposed=True, bias=self._wt["ap_b"])
        self._draw(r["logits_pad"][:, :net.n_action], t)

    # ---- what depends on the form of the policy head (factored.FactoredCnnA2CRunner states its own) ----------------------------------
    def _draw(self, logits, t):
        """Step t's actions from its logits (GPU), into act_buf[t]."""
        from . import _agent_capi as A

        A.sample_actions(logits, self.u_buf[t], out=self.act_buf[t])

    def _draw_reference(self, t):
        """Step t's actions on the CPU path: the plain PyTorch forward and draw."""
        return sample_actions(self.net.actor_only(self.idx_buf[t]), uniforms=self.u_buf[t])

    def _loss_workspace(self):
        from . import _agent_capi as A

        return A.loss_grad_workspace(self.net.n_action, self.dev)

    def _loss_grad(self, logits, v, target, actions, dv, dbias, loss, ws):
        from . import _agent_capi as A

        A.a2c_loss_grad(logits, v, target, actions, self.beta, dv, dbias, loss, ws)

    @torch.no_grad()
    def collect(self):
        """One rollout: per step conv1 from idx[t] -> conv2 -> conv3 -> dense -> policy head -> action draw -> env.step -> idx[t + 1].
        Returns (idx [T,N,K], actions [T,N], rewards [T,N], bootstrap [N]) -- views valid until the next collect()."""
        env, T = self.env, self.T
        self._check_reward_spec()
        self.u_buf.copy_(torch.rand(self.u_buf.shape, device=self.dev, dtype=torch.float32, generator=self.gen))
        self._refresh_transposed()
        self.idx_buf[0].copy_(self.idx_buf[T])
        cuda = self.dev.type == "cuda"
        for t in range(T):
            if cuda:
                self._policy_step(t)
            else:
                self.act_buf[t] = self._draw_reference(t)
            env.step(self.act_buf[t], reward_out=self.rew_buf[t])
            self._after_step(t)
        done = env.out["done"].bool()
        return self._end_rollout(done, bool(done.any()))

    def _ensure_update_buffers(self, chunk, K_nodes):
        from . import _agent_capi as A
        from . import _cnn_capi as K

        if self._upd is not None and self._upd["chunk"] == chunk:
            return self._upd
        self._upd = None
        G, dev, na = self.G, self.dev, self.net.n_action
        ldl = (na + 15) // 16 * 16
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        b = {"chunk": chunk, "logits_pad": torch.zeros((chunk, ldl), device=dev), "v": f(chunk), "dv": f(chunk), "dh": f(chunk, DENSE),
             "dflat": _act(chunk, G - 12, dev), "dc2": _act(chunk, G - 8, dev), "dc1": _act(chunk, G - 4, dev),
             "loss": torch.zeros(3, dtype=torch.float64, device=dev), "loss_sum": torch.zeros(3, dtype=torch.float64, device=dev),
             "t_ap_k": f(DENSE, na), "t_ap_b": f(na), "t_d2_b": f(DENSE), "t_v_k": f(DENSE),
             "ws_loss": self._loss_workspace(), "ws_relu": A.relu6_bwd_workspace(DENSE, dev), "ws": {}}
        for p in ("a", "c"):
            b[p] = {"c1": _act(chunk, G - 4, dev), "c2": _act(chunk, G - 8, dev), "c3": _act(chunk, G - 12, dev), "h": f(chunk, DENSE)}
        self._upd = b
        return b

    def _workspaces(self, b, mc):
        """Workspaces for a chunk of mc samples (their sizes need not grow with mc: each buffer grows to the largest request)."""
        from . import _agent_capi as A
        from . import _cnn_capi as K

        G, la, lk = self.G, A.load(), K.load()
        need = {"dense": lk.uavcnn_dense_fwd_workspace_bytes(mc, flat_dim(G)), "c1": lk.uavcnn_conv1_wgrad_workspace_bytes(mc, self.B),
                "c2": lk.uavcnn_conv5_wgrad_workspace_bytes(mc, G - 4), "c3": lk.uavcnn_conv5_wgrad_workspace_bytes(mc, G - 8),
                "tn": la.uavagent_gemm_tn_workspace_bytes(mc, self.net.n_action), "cs": la.uavagent_gemm_rows_workspace_bytes(mc)}
        ws = b["ws"]
        for k, n in need.items():
            if k not in ws or ws[k].numel() < n:
                ws[k] = K.workspace(n, self.dev)
        return ws

    def _trunk_backward(self, pre, idx, act, b, mc, dh):
        """One trunk backwards from d(dense output) dh (relu6 mask applied): every weight gradient is ADDED to the flat gradient."""
        from . import _cnn_capi as K

        net, gv, G = self.net, self.flat.gv, self.G
        c1, c2, c3 = act["c1"][:mc], act["c2"][:mc], act["c3"][:mc]
        dflat, dc2, dc1 = b["dflat"][:mc], b["dc2"][:mc], b["dc1"][:mc]
        n = "la2" if pre == "a" else "lc2"
        K.dense_wgrad(c3.view(mc, -1), dh, gv["%s_%s_k" % (pre, n)], accumulate=True)
        K.dense_dx(dh, getattr(net, "%s_%s_k" % (pre, n)), c3.view(mc, -1), dflat.view(mc, -1))
        ws = b["ws"]
        K.conv5_wgrad(c2, dflat, gv[pre + "_conv3_k"], gv[pre + "_conv3_b"], ws["c3"], accumulate=True)
        K.conv5(dflat, self._wt[pre + "_conv3_flip"], dc2, pad=4, mask=c2)
        K.conv5_wgrad(c1, dc2, gv[pre + "_conv2_k"], gv[pre + "_conv2_b"], ws["c2"], accumulate=True)
        K.conv5(dc2, self._wt[pre + "_conv2_flip"], dc1, pad=4, mask=c1)
        K.conv1_wgrad(idx, self.B, G, dc1, gv[pre + "_conv1_k"], gv[pre + "_conv1_b"], ws["c1"], accumulate=True)

    @torch.no_grad()
    def update_fused(self, idx_buf, act_buf, rew_buf, boot):
        """The update with the hand-derived backward pass, chunk by chunk: both trunks forwards (activations kept), the loss gradient
        (scaled by chunk / M: the loss stays the mean over all T*N samples), both trunks backwards into the flat gradient; then one TF1
        RMSProp step per trunk."""
        from . import _agent_capi as A
        from . import _cnn_capi as K

        net, fl, gv = self.net, self.flat, self.flat.gv
        T, N, Kn = idx_buf.shape
        M = T * N
        chunk = min(self.update_chunk, M)
        b = self._ensure_update_buffers(chunk, Kn)
        target = self._nstep_targets(rew_buf, boot, True).reshape(M)
        idx, act = idx_buf.reshape(M, Kn).contiguous(), act_buf.reshape(M).contiguous()
        self._refresh_transposed()
        fl.zero_grad()
        b["loss_sum"].zero_()
        wt, na = self._wt, net.n_action
        for s in range(0, M, chunk):
            e = min(M, s + chunk)
            mc, w = e - s, (e - s) / M
            ix = idx[s:e]
            ta, tc = b["a"], b["c"]
            ws = self._workspaces(b, mc)
            K.conv1_from_idx(ix, self.B, self.G, net.a_conv1_k, net.a_conv1_b, ta["c1"][:mc], net.c_conv1_k, net.c_conv1_b, tc["c1"][:mc])
            for p, tr in (("a", ta), ("c", tc)):
                _trunk_tail(net, p, tr["c1"][:mc], tr["c2"][:mc], tr["c3"][:mc], tr["h"][:mc], ws["dense"])
            lp = b["logits_pad"][:mc]
            A.gemm_rows(ta["h"][:mc], wt["ap_t"], lp, w_transposed=True, bias=wt["ap_b"])
            v, dv = b["v"][:mc], b["dv"][:mc]
            A.rowdot(tc["h"][:mc], net.c_v_k.reshape(-1), net.c_v_b, v)
            self._loss_grad(lp[:, :na], v, target[s:e], act[s:e], dv, b["t_ap_b"], b["loss"], b["ws_loss"])
            b["loss_sum"].add_(b["loss"], alpha=w)
            lp.mul_(w)
            dv.mul_(w)
            gv["a_ap_b"].add_(b["t_ap_b"], alpha=w)
            gv["c_v_b"].add_(b["loss"][2:3].to(torch.float32), alpha=w)
            # actor: head (libuavagent), then the trunk
            dh = b["dh"][:mc]
            A.gemm_tn(ta["h"][:mc], lp[:, :na], b["t_ap_k"], ws["tn"])
            gv["a_ap_k"].add_(b["t_ap_k"])
            A.gemm_rows(lp, wt["ap_p"], dh, w_transposed=True, relu6_mask_h=ta["h"][:mc], colsum_out=b["t_d2_b"], workspace=ws["cs"])
            gv["a_la2_b"].add_(b["t_d2_b"])
            self._trunk_backward("a", ix, ta, b, mc, dh)
            # critic: value head + relu6 (libuavagent), then the trunk
            A.relu6_bwd(None, tc["h"][:mc], dh, DENSE, b["t_d2_b"], b["ws_relu"], dv=dv, w3=net.c_v_k.reshape(-1), dw3_out=b["t_v_k"])
            gv["c_lc2_b"].add_(b["t_d2_b"])
            gv["c_v_k"].add_(b["t_v_k"].view(DENSE, 1))
            self._trunk_backward("c", ix, tc, b, mc, dh)
        self._optimizer_step(1.0)                                    # (one process only: nothing to exchange)
        loss, clip_stats = self._read_loss(b["loss_sum"], 1.0)       # (synchronises)
        self.stats = {"a_loss": float(loss[0]), "c_loss": float(loss[1]), "mean_reward": float(rew_buf.mean()), "grad_elems": fl.n_real,
                      "running_r": self.running_r, "allreduce_ms": None, "chunks": (M + chunk - 1) // chunk}
        self.stats.update(clip_stats)
        return self.stats

    def state_dict(self):
        sd = super().state_dict()
        sd["net"] = self.NET_KIND
        return sd
