"""Batched greedy evaluation of a trained actor: the loop of the reference's main_test.py (:46-113) for N envs at once.

main_test.py steps ``step_test`` with ``tf.argmax(a_prob)`` (:68,73) and keeps the reward, the outage and ``current_BS_sinr`` of every
step.  Here the loop stays on the device: per step the actor's first layer from the compact observation, the greedy policy head
(libuavagent.so), the env step (libuavenv.so) and one launch that folds the step's outputs into per-env totals and a serving-SINR
histogram (uavenv_eval_accumulate) -- 4096 envs x 2001 steps x 40 UEs of SINR would be 1.3 GB if kept.  No host synchronisation and
no allocation inside the loop.

    ev = GreedyEvaluator(env, net)                       # env: BatchedMobiEnv, net: agent.ACNet or cnn_agent.CnnACNet
    res = ev.run(2000)                                   # group mobility, from the env's current state
    res = ev.run(2000, trace=cells)                      # read_trace: cells int16 [2001, N, U, 2] or [2001, U, 2] (every env the same)

The greedy choice is argmax(logits), ``greedy_reference`` below; it equals tf.argmax(softmax(logits)) except where two different
logits round to the same float32 probability.
"""
import numpy as np
import torch

from .agent import ACNet


def greedy_reference(logits, n_actions):
    """The greedy rule of the HIP kernels in NumPy: for every row of ``logits`` [M, >= n_actions] the first index a < n_actions whose
    logit no other exceeds.  Comparison is strict, so of equal logits the lowest index wins (np.argmax / tf.argmax); a NaN never wins;
    a row of NaNs only gives 0; columns >= n_actions (the kernels' zero padding) are ignored.  Returns int64 [M]."""
    l = np.asarray(logits)
    if l.ndim != 2 or not 1 <= int(n_actions) <= l.shape[1]:
        raise ValueError("logits must be [M, >= n_actions]")
    l = l[:, :int(n_actions)]
    valid = ~np.isnan(l)
    best = np.where(valid, l, -np.inf).max(axis=1, keepdims=True)
    hit = valid & (l == best)
    return hit.argmax(axis=1).astype(np.int64)          # (no hit at all: argmax of all-False = 0)


class GreedyEvaluator:
    """``run(n_steps, trace=None, keep=("reward", "actions"))`` evaluates ``net`` greedily on every env of ``env``.

    Routing: an ACNet of the reference's widths (200 hidden units, 577..640 actions) takes the fused greedy head
    (uavagent_actor_head_greedy_f32); any other ACNet width and CnnACNet compute their logits as their rollout does and pick with
    uavagent_argmax_rows_f32; a factored.FactoredCnnACNet takes the CNN route with the greedy digit per UAV
    (uavagent_choose_factored_f32 without uniforms) in its place.  The MLP's first layer comes straight from the compact observation (uavagent_first_layer_from_obs_f32,
    actor table only), which bounds it to nBS + nUE <= 64 like the index-list gather.  A factored.FactoredACNet takes the MLP route up to 256
    nodes (the wide from-obs gather above 64), its two dense layers through uavagent_gemm_rows_f32 and the greedy digit per UAV.  ``hist`` = (lo, hi, bins) of the serving-SINR histogram in dB."""

    def __init__(self, env, net, hist=(-50.0, 100.0, 150), mask_margin=None):
        from . import _agent_capi as A

        if env.device.type != "cuda":
            raise A.UavAgentError("GreedyEvaluator needs the env's GPU (there is no CPU path)")
        A.load()
        self.env, self.dev = env, env.device
        self.net = net.to(self.dev)
        # mask_margin (a factored.FactoredACNet only): the greedy digit per UAV among the digits env.action_mask(margin)
        # allows -- this evaluator keeps no index list, so the bits come from the env and go to the masking pass as they are
        if mask_margin is not None:
            from .factored import check_mask_margin

            mask_margin = check_mask_margin(mask_margin)
            if not (isinstance(net, ACNet) and getattr(net, "factored", False)):
                raise ValueError("GreedyEvaluator: mask_margin serves a factored.FactoredACNet only")
            self._mask_bits = torch.empty((env.n_envs, env.nBS), dtype=torch.uint8, device=self.dev)
        self.mask_margin = mask_margin
        self.acc = env.eval_accumulators(hist)
        N, U, B = env.n_envs, env.nUE, env.nBS
        NA = int(net.n_action)
        self._factored = bool(getattr(net, "factored", False))     # factored.FactoredCnnACNet: n_action = heads x digits, not joint actions
        if self._factored:
            if net.n_heads != B or net.joint_actions != env.action_space_dim:
                raise ValueError("the net has %d heads of %d actions, the env %d UAVs and %d joint actions" % (
                    net.n_heads, net.n_act, B, env.action_space_dim))
        elif NA != env.action_space_dim:
            raise ValueError("the net has %d actions, the env %d" % (NA, env.action_space_dim))
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.dev)
        self._ldl = (NA + 15) // 16 * 16
        self._logits_pad = torch.zeros((N, self._ldl), dtype=torch.float32, device=self.dev)
        self._idx = torch.empty((N, B + U), dtype=torch.int64, device=self.dev)
        self._trace_stage = torch.empty((N, U, 2), dtype=torch.int16, device=self.dev)
        self._bufs = {}                                    # T -> (actions [T, N] or None, reward [T, N] or None)
        if isinstance(net, ACNet):
            H = int(net.a_w2.shape[0])
            self.kind = "mlp_factored" if self._factored else ("mlp_fused" if (H == 200 and 576 < NA <= 640) else "mlp")
            if self._factored and B + U > A.WIDE_NODES:
                raise ValueError("GreedyEvaluator: the wide first-layer gather holds nBS + nUE <= 256 nodes (got %d)" % (B + U))
            if not self._factored and B + U > 64:      # (building an index list first would not help: uavagent_first_layer_f32 has the same bound)
                raise ValueError("GreedyEvaluator: the MLP's first-layer gather holds one node per lane, nBS + nUE <= 64 (got %d); "
                                 "larger shapes need the CNN actor" % (B + U))
            self._h1, self._h2 = f(N, H), f(N, H)
            if self.kind in ("mlp_fused", "mlp_factored"):
                self._w2t = f(H, H)
                self._w3t = torch.zeros((self._ldl, H), dtype=torch.float32, device=self.dev)
                self._b3p = torch.zeros(self._ldl, dtype=torch.float32, device=self.dev)
        else:
            from .cnn_agent import DENSE, CnnACNet, _act, flat_dim

            if not isinstance(net, CnnACNet):
                raise TypeError("GreedyEvaluator evaluates an agent.ACNet or a cnn_agent.CnnACNet")
            from . import _cnn_capi as K

            G = env.grid_n
            self.kind = "cnn"
            self._c = (_act(N, G - 4, self.dev), _act(N, G - 8, self.dev), _act(N, G - 12, self.dev))
            self._h1 = f(N, DENSE)
            self._ws = K.dense_fwd_workspace(N, flat_dim(G), self.dev)
            self._apt = torch.zeros((self._ldl, DENSE), dtype=torch.float32, device=self.dev)
            self._apb = torch.zeros(self._ldl, dtype=torch.float32, device=self.dev)

    @torch.no_grad()
    def _refresh_weights(self):
        """The transposed / padded copies the kernels read, from the parameters as they are now."""
        net, NA = self.net, self.net.n_action
        if self.kind in ("mlp_fused", "mlp_factored"):
            self._w2t.copy_(net.a_w2.t())
            self._w3t[:NA].copy_(net.a_w3.t())
            self._b3p[:NA].copy_(net.a_b3)
        elif self.kind == "cnn":
            self._apt[:NA].copy_(net.a_ap_k.t())
            self._apb[:NA].copy_(net.a_ap_b)

    @torch.no_grad()
    def _choose(self, act):
        """Greedy actions of every env for the observation the env holds now, into ``act`` int64 [N]."""
        from . import _agent_capi as A

        env, net, NA = self.env, self.net, self.net.n_action
        obs = env.observation()
        if self.kind == "cnn":
            from . import _cnn_capi as K
            from .cnn_agent import _trunk_tail

            A.obs_indices(obs, env.grid_n, env.nBS, out=self._idx)
            K.conv1_from_idx(self._idx, env.nBS, env.grid_n, net.a_conv1_k, net.a_conv1_b, self._c[0])
            _trunk_tail(net, "a", self._c[0], self._c[1], self._c[2], self._h1, self._ws)
            A.gemm_rows(self._h1, self._apt, self._logits_pad, w_transposed=True, bias=self._apb)
            if self._factored:
                A.choose_factored(self._logits_pad[:, :NA], None, net.n_heads, net.n_act, out=act)
            else:
                A.argmax_rows(self._logits_pad[:, :NA], out=act)
            return
        from_obs = A.first_layer_from_obs if env.nBS + env.nUE <= A.NARROW_NODES else A.first_layer_from_obs_wide
        from_obs(obs, env.grid_n, net.a_w1, net.a_b1, None, None, self._h1, None)                     # actor table only, relu6
        if self.kind == "mlp_factored":
            A.gemm_rows(self._h1, self._w2t, self._h2, w_transposed=True, bias=net.a_b2, relu6=True)
            A.gemm_rows(self._h2, self._w3t, self._logits_pad, w_transposed=True, bias=self._b3p)
            if self.mask_margin is not None:
                A.mask_move_logits(self._logits_pad[:, :NA], net.n_heads, bits=env.action_mask(self.mask_margin, out=self._mask_bits))
            A.choose_factored(self._logits_pad[:, :NA], None, net.n_heads, net.n_act, out=act)
        elif self.kind == "mlp_fused":
            A.actor_head_greedy(self._h1, self._w2t, net.a_b2, self._w3t, self._b3p, NA, self._h2, self._logits_pad, act)
        else:
            logits = self._logits_pad[:, :NA]
            torch.addmm(net.a_b2, self._h1, net.a_w2, out=self._h2).clamp_(0.0, 6.0)
            torch.addmm(net.a_b3, self._h2, net.a_w3, out=logits)
            A.argmax_rows(logits, out=act)

    def _trace_on_device(self, trace, n_steps):
        N, U = self.env.n_envs, self.env.nUE
        t = torch.as_tensor(trace)
        if t.dtype != torch.int16 or t.dim() not in (3, 4) or tuple(t.shape[-2:]) != (U, 2) or (t.dim() == 4 and t.shape[1] != N):
            raise ValueError("trace must be int16 [T + 1, N, U, 2] or [T + 1, U, 2]")
        if t.shape[0] < n_steps + 1:
            raise ValueError("trace has %d rows, %d steps need %d (row 0 is the reset's)" % (t.shape[0], n_steps, n_steps + 1))
        return t[:n_steps + 1].to(self.dev).contiguous()

    @torch.no_grad()
    def run(self, n_steps, trace=None, keep=("reward", "actions"), after_step=None, rates=False):
        """``n_steps`` greedy steps of every env.  Group mobility (``trace`` None): from the env's current state.  Trace mode: row 0 of
        ``trace`` goes to reset_trace and row t + 1 to step t, the indexing main_test.py ends up with.  The accumulators are zeroed
        first.  Returns a dict: ``actions`` int64 [T, N] / ``reward`` float32 [T, N] when named in ``keep`` (overwritten by the next run
        of the same length), the accumulator tensors (reward_sum, mean_sinr_sum, n_out_sum, steps, sinr_hist, sinr_nan),
        ``outage_fraction`` = n_out_sum / (steps * nUE) float64 [N] and ``hist_edges`` float64 [bins + 1].  Asynchronous.
        ``after_step(t)``: an optional host callback behind step t's launches (tools/run_eval.py takes its SINR maps there); what it
        synchronises or allocates is its own affair.  ``rates``: one link_rates call per step into rate accumulators; the result gains
        ``dl_rate_mean`` / ``ul_rate_mean`` float64 [N], the per-env mean serving rates (Mb/s per channel) averaged over the steps.
        Without it the loop issues exactly the launches it always did."""
        env, T, N = self.env, int(n_steps), self.env.n_envs
        keep = tuple(keep)
        if set(keep) - {"reward", "actions"}:
            raise ValueError("keep may name 'reward' and 'actions'")
        if T not in self._bufs:
            if len(self._bufs) > 4:
                self._bufs.clear()
            self._bufs[T] = (torch.empty((T, N), dtype=torch.int64, device=self.dev), torch.empty((T, N), dtype=torch.float32, device=self.dev))
        act_buf, rew_buf = self._bufs[T]
        keep_r = "reward" in keep
        tr = None
        if trace is not None:
            tr = self._trace_on_device(trace, T)
            per_env = tr.dim() == 4
            stage = self._trace_stage
            cells = lambda t: tr[t] if per_env else stage.copy_(tr[t].unsqueeze(0).expand_as(stage))
            env.reset_trace(cells(0))
        self._refresh_weights()
        self.acc.zero_()
        reward = env.out["reward"]
        racc = None
        if rates:
            if getattr(self, "_racc", None) is None:
                self._racc = env.rate_accumulators()
            racc = self._racc
            for v in racc.values():
                v.zero_()
        # ---- the loop: no synchronisation, no allocation ----
        for t in range(T):
            a = act_buf[t]
            self._choose(a)
            if tr is None:
                env.step(a)
            else:
                env.step_trace(a, cells(t + 1))
            if keep_r:
                rew_buf[t].copy_(reward)
            env.eval_accumulate(self.acc)
            if racc is not None:
                env.link_rates(want=(), accumulate=racc)
            if after_step is not None:
                after_step(t)
        res = dict(self.acc.tensors())
        if "actions" in keep:
            res["actions"] = act_buf
        if keep_r:
            res["reward"] = rew_buf
        res["outage_fraction"] = self.acc.n_out_sum.to(torch.float64) / (self.acc.steps.to(torch.float64) * env.nUE)
        res["hist_edges"] = torch.as_tensor(self.acc.hist_edges())
        if racc is not None:
            steps = racc["rate_steps"].to(torch.float64)
            res["dl_rate_mean"] = racc["dl_rate_mean_sum"] / steps
            res["ul_rate_mean"] = racc["ul_rate_mean_sum"] / steps
        return res
