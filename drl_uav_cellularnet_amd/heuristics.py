"""The reference's hand-written "SINR-gradient" controller (gradient.py:14-37) on top of the drop-in MobiEnvironment:
a policy-free, deterministic-given-the-seed end-to-end driver (SURVEY.md section 8 f, row 3).  Host-side logic only;
every env operation (deepcopy, step_test) goes through the HIP path.

For a batch the controller itself is a HIP kernel (BatchedMobiEnv.gradient_actions / step_gradient); here are its NumPy statement of
the rule (side_rule) and the same decision built from a twin handle and the ordinary step (gradient_actions_reference), which is what
the kernel is tested and timed against and what serves the shapes the kernel refuses (n_ue > 64).

The one-step search policy (BatchedMobiEnv.search_actions / step_search: the best of all joint actions per env) has the same pair
here: search_rule and search_actions_reference; so has the per-UAV coordinate-search policy (coordinate_actions / step_coordinate:
each UAV's best cell in turn): coordinate_rule and coordinate_actions_reference.

Reward-aware look-ahead (``shaped=True`` of search_actions / coordinate_actions): the two *_actions_reference functions read the twin's
``reward`` / ``reward_f64``, which the twin's post-step kernel has shaped when the twin carries a reward spec -- so with such a twin
(``env.clone()`` of an env with a spec) they return SHAPED tables and are the yardstick of the shaped kernels as they stand.
shaped_candidate_value states in NumPy what a shaped kernel computes for one candidate from the quantities it holds."""
import warnings
from copy import deepcopy

import numpy as np


def side_means(current_bs_sinr, ue_loc, bs_xy):
    """dir_grad of gradient.py:27-31 for one UAV: mean serving SINR of the UEs with x > bx, x <= bx, y > by, y <= by
    (NaN for an empty side, exactly like np.mean of an empty selection)."""
    out = np.full(4, np.nan)
    sel = (ue_loc[:, 0] > bs_xy[0], ue_loc[:, 0] <= bs_xy[0], ue_loc[:, 1] > bs_xy[1], ue_loc[:, 1] <= bs_xy[1])
    for k, m in enumerate(sel):
        if m.any():
            out[k] = np.mean(current_bs_sinr[m])
    return out


def choose_act_gradient(actual_env, n_act=5):
    """Choose_Act_Gradient (gradient.py:14-37): look one step ahead on a deep copy with every UAV staying (action
    n_act**nBS - 1 = "44..4"), then move each UAV towards the side whose UEs have the lowest mean serving SINR
    (digit 0: +x, 1: -x, 2: +y, 3: -y; ue_mobility.py:221-235).  The caller's env is not modified."""
    virtual_env = deepcopy(actual_env)                                   # :15
    stay = n_act ** actual_env.nBS - 1                                   # 624 for 4 UAVs (:17)
    virtual_env.step_test(stay, False)
    sinr, bs_loc, ue_loc = virtual_env.channel.current_BS_sinr, virtual_env.bsLoc, virtual_env.ueLoc   # :20-22
    action = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for i_bs in range(len(bs_loc)):                                  # :26-32
            digit = int(np.nanargmin(side_means(sinr, ue_loc, bs_loc[i_bs])))
            action = action * n_act + digit                              # most significant digit -> UAV 0 (:34)
    return action


def run_gradient_policy(env, n_steps, reset_every=2000):
    """The loop of gradient.py:56-86 without its file output: returns (rewards, actions)."""
    env.reset()
    rewards, actions = [], []
    for step in range(n_steps):
        a = choose_act_gradient(env)
        _, r, done, _ = env.step_test(a, False)
        rewards.append(r)
        actions.append(a)
        if (step + 1) % reset_every == 0:
            env.reset()
    return np.array(rewards), np.array(actions)


def side_rule(cur_sinr, ue_xy, bs_xy, n_act=5):
    """The rule of gradient.py:26-34 for a batch, in NumPy float64: cur_sinr [N, U], ue_xy [N, U, 2], bs_xy [N, B, 2] ->
    (side means [N, B, 4] with NaN for an empty side, joint actions int64 [N]).  Per env and UAV it is side_means() and
    np.nanargmin, so each mean is the very np.mean the reference takes."""
    cur = np.asarray(cur_sinr, np.float64)
    ue, bs = np.asarray(ue_xy), np.asarray(bs_xy)
    N, B = bs.shape[0], bs.shape[1]
    means = np.empty((N, B, 4))
    actions = np.empty(N, np.int64)
    for e in range(N):
        a = 0
        for b in range(B):
            means[e, b] = side_means(cur[e], ue[e], bs[e, b])
            a = a * n_act + int(np.nanargmin(means[e, b]))               # most significant digit -> UAV 0 (:34)
        actions[e] = a
    return means, actions


def gradient_actions_reference(env, twin, side_means=False):
    """choose_act_gradient for every env of a BatchedMobiEnv, from the pieces the env has always had: ``twin`` (a second
    BatchedMobiEnv of the same shape, seed and env_id_base, e.g. ``env.clone()``, kept by the caller) takes a copy of the state,
    steps once with every UAV staying, and the rule runs as torch ops on the twin's outputs.  ``env`` is not modified.  Any shape,
    n_ue > 64 included.  Returns int64 [N] on the device (and the side means [N, B, 4] float64 when asked)."""
    import torch

    buf = getattr(twin, "_gradient_state_buf", None)
    if buf is None:
        buf = twin._gradient_state_buf = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
        twin._gradient_stay = torch.full((env.n_envs,), env.N_ACT ** env.nBS - 1, dtype=torch.int64, device=env.device)
    env.copy_state_to(buf)
    twin.copy_state_from(buf)
    twin.step(twin._gradient_stay)
    o = twin.out
    cur = o["cur_sinr_f64"] if "cur_sinr_f64" in o else o["cur_sinr"].double()            # [N, U]
    ue, bs = o["ue_xy"].int(), o["bs_xy"]                                                  # [N, U, 2], [N, B, 2]
    gt_x = ue[:, None, :, 0] > bs[:, :, None, 0]                                           # [N, B, U]
    gt_y = ue[:, None, :, 1] > bs[:, :, None, 1]
    sel = torch.stack((gt_x, ~gt_x, gt_y, ~gt_y), dim=2)                                   # [N, B, 4, U]
    cnt = sel.sum(-1)
    means = (sel * cur[:, None, None, :]).sum(-1) / cnt                                    # 0 / 0 = NaN: an empty side
    digit = torch.where(cnt > 0, means, torch.full_like(means, float("inf"))).argmin(-1)   # nanargmin (no side mean is infinite)
    w = env.N_ACT ** torch.arange(env.nBS - 1, -1, -1, device=env.device, dtype=torch.int64)
    actions = (digit * w).sum(-1)
    return (actions, means) if side_means else actions


def shaped_candidate_value(spec, sum_cur, n_out, cur, cells, n_ue, checked=True):
    """The value a shaped look-ahead gives one candidate joint action (include/uavenv.h, "Reward-aware look-ahead"): ``sum_cur`` the
    per-env sum of the serving SINRs, ``n_out`` the newly outaged walkers, ``cur`` [U] the serving SINRs before any handover, ``cells``
    [B, 2] where BS_move leaves the UAVs.  rewards.reward_reference on mean = sum_cur * (1 / U) -- the product the step's mean_sinr is,
    not sum_cur / U -- with, when not ``checked``, mean and cur rounded through float32 first (what the post-step kernel reads behind a
    step with float32 outputs).  -> (value float64, terms float64 [4])."""
    from . import rewards

    mean = np.float64(sum_cur) * (np.float64(1.0) / np.float64(n_ue))
    cur = None if cur is None else np.asarray(cur, np.float64)
    if not checked:
        mean = np.float64(np.float32(mean))
        cur = None if cur is None else cur.astype(np.float32).astype(np.float64)
    return rewards.reward_reference(spec, mean, n_out, cur, cells, n_ue)


def frozen_uavs(bs_xy, min_bs_dist):
    """UAVs BS_move will not move again: those with another UAV within ``min_bs_dist`` cells (ue_mobility.py:256-266; a UAV's own moves
    cannot end it, its pre-move cell is what is tested).  bs_xy [..., B, 2] integer cells -> bool [..., B]."""
    bs = np.asarray(bs_xy, np.int64)
    d2 = ((bs[..., :, None, :] - bs[..., None, :, :]) ** 2).sum(-1)
    B = bs.shape[-2]
    return ((d2 <= int(min_bs_dist) ** 2) & ~np.eye(B, dtype=bool)).any(-1)


MOVE_DELTAS = ((1, 0), (-1, 0), (0, 1), (0, -1))      # digits 0 .. 3 of BS_move in units of bs_step (ue_mobility.py:221-235); 4 = stay


def move_mask(bs_xy, grid_n, bs_step, min_bs_dist, margin):
    """The move mask of DESIGN.md section 27 (csrc/move_mask.h states it for the kernels), integers only: bs_xy [..., B, 2] integer cells ->
    bool [..., B, 5].  For UAV b at c_b and digit d < 4 with dest = c_b moved by bs_step:
        wall   = BS_move's guard fails (x + s < G, x - s > 1, y + s < G, y - s > 1)
        frozen = some j != b has |c_b - c_j|^2 <= min_bs_dist^2 (frozen_uavs)
        crowd  = margin > 0 and some j != b has |dest - c_j|^2 <= margin^2
        allowed[b, d] = not (wall or frozen or crowd);  allowed[b, 4] = True.
    margin = 0: "UAV b taking d while everybody else stays changes b's cell".  margin >= min_bs_dist + bs_step: from a layout without a
    frozen pair, no joint action of allowed digits freezes a UAV or is left uncommitted."""
    bs = np.asarray(bs_xy, np.int64)
    G, s, m = int(grid_n), int(bs_step), int(margin)
    if m < 0:
        raise ValueError("margin must be >= 0")
    B = bs.shape[-2]
    x, y = bs[..., 0], bs[..., 1]
    ok = np.stack([x + s < G, x - s > 1, y + s < G, y - s > 1], axis=-1)                   # [..., B, 4]
    ok &= ~frozen_uavs(bs, min_bs_dist)[..., None]
    if m > 0 and B > 1:
        dest = bs[..., :, None, :] + s * np.asarray(MOVE_DELTAS, np.int64)                 # [..., B, 4, 2]
        d2 = ((dest[..., :, :, None, :] - bs[..., None, None, :, :]) ** 2).sum(-1)         # [..., B, 4, B(j)]
        near = (d2 <= m * m) & ~np.eye(B, dtype=bool)[:, None, :]
        ok &= ~near.any(-1)
    return np.concatenate([ok, np.ones(ok.shape[:-1] + (1,), dtype=bool)], axis=-1)


def mask_bits(allowed):
    """bool [..., 5] -> uint8 [...], bit d = digit d allowed: the storage form of uavenv_action_mask and uavagent_mask_move_logits_f32."""
    a = np.asarray(allowed, bool)
    return (a * (1 << np.arange(a.shape[-1]))).sum(-1).astype(np.uint8)


def mask_bits_to_allowed(bits):
    """uint8 [...] mask bits (NumPy array or torch tensor) -> bool [..., 5] of the same kind."""
    if isinstance(bits, np.ndarray):
        return ((bits[..., None] >> np.arange(5, dtype=np.uint8)) & 1).astype(bool)
    import torch

    sh = torch.arange(5, device=bits.device, dtype=torch.int32)
    return ((bits.to(torch.int32).unsqueeze(-1) >> sh) & 1).bool()


def search_rule(rewards):
    """The one-step search policy's choice from a table of action values: rewards [N, A] -> int64 [N], per row the FIRST maximum
    (the lowest action among equal rewards).  A NaN never wins; a row of NaNs gives 0."""
    r = np.asarray(rewards, np.float64)
    return np.where(np.isnan(r), -np.inf, r).argmax(axis=1).astype(np.int64)           # np.argmax returns the first maximum


def search_actions_reference(env, twin):
    """The search of BatchedMobiEnv.search_actions from the pieces the env has always had: ``twin`` (a second BatchedMobiEnv of the
    same shape, seed and env_id_base, e.g. ``env.clone()``, kept by the caller) takes a copy of the state before EACH of the
    N_ACT ** nBS joint actions and steps with it for every env at once; the rewards (``reward_f64`` when the twin has float64
    outputs, else the float32 ``reward``) fill the table.  ``env`` is not modified.  Any shape, n_ue > 64 included.  Returns
    (actions int64 [N], table float64 [N, A]) on the device: the yardstick for tests and timing."""
    import torch

    A = env.N_ACT ** env.nBS
    buf = getattr(twin, "_search_state_buf", None)
    if buf is None:
        buf = twin._search_state_buf = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
        twin._search_act = torch.empty((env.n_envs,), dtype=torch.int64, device=env.device)
    env.copy_state_to(buf)
    table = torch.empty((env.n_envs, A), dtype=torch.float64, device=env.device)
    key = "reward_f64" if "reward_f64" in twin.out else "reward"
    for a in range(A):
        twin.copy_state_from(buf)
        twin._search_act.fill_(a)
        twin.step(twin._search_act)
        table[:, a] = twin.out[key]
    nan_low = torch.where(torch.isnan(table), torch.full_like(table, float("-inf")), table)
    best = nan_low.max(dim=1, keepdim=True).values
    idx = torch.arange(A, device=env.device).expand_as(table)
    actions = torch.where(nan_low == best, idx, torch.full_like(idx, A)).min(dim=1).values      # the lowest index that holds the maximum
    return actions, table


def coordinate_rule(rewards, n_act=5):
    """The coordinate-search policy's choice from a table whose rows are already conditional on the earlier choices: rewards
    [N, B, n_act] -> (digits int64 [N, B], joint actions int64 [N]).  Per row the first maximum in the order stay (digit n_act - 1),
    0, 1, ..: a UAV moves only for a strictly higher reward than staying, the lowest digit wins among equal moves, a NaN never
    wins and a row of NaNs gives stay.  Joint action = sum digit_b n_act^(B-1-b), UAV 0 the most significant digit."""
    r = np.asarray(rewards, np.float64)
    N, B, A = r.shape
    order = np.array([A - 1] + list(range(A - 1)))
    v = np.where(np.isnan(r), -np.inf, r)[:, :, order]
    digits = order[v.argmax(axis=2)].astype(np.int64)                                   # np.argmax returns the first maximum
    w = np.array([n_act ** (B - 1 - b) for b in range(B)], dtype=object)                # exact beyond 2^53 as well
    actions = np.array([int((row.astype(object) * w).sum()) for row in digits], dtype=np.int64).reshape(N)
    return digits, actions


def coordinate_actions_reference(env, twin):
    """The search of BatchedMobiEnv.coordinate_actions from the pieces the env has always had: ``twin`` (a second BatchedMobiEnv of
    the same shape, seed and env_id_base, e.g. ``env.clone()``, kept by the caller) takes a copy of the state before each of the
    4 nBS + 1 joint actions -- per env (c_0 .. c_{i-1}, d, 4 .. 4) -- and steps with it; the rewards (``reward_f64`` when the twin
    has float64 outputs, else the float32 ``reward``) fill the table.  ``env`` is not modified.  Any shape.  Returns (actions int64
    [N], table float64 [N, B, 5], best reward float64 [N]) on the device: the yardstick for tests and timing."""
    import torch

    B, A, N = env.nBS, env.N_ACT, env.n_envs
    stay_d = A - 1
    buf = getattr(twin, "_coord_state_buf", None)
    if buf is None:
        buf = twin._coord_state_buf = torch.empty(env._lay.total_bytes, dtype=torch.uint8, device=env.device)
    env.copy_state_to(buf)
    key = "reward_f64" if "reward_f64" in twin.out else "reward"
    w = A ** torch.arange(B - 1, -1, -1, device=env.device, dtype=torch.int64)
    digits = torch.full((N, B), stay_d, dtype=torch.int64, device=env.device)
    table = torch.empty((N, B, A), dtype=torch.float64, device=env.device)

    def value(dg):
        twin.copy_state_from(buf)
        twin.step((dg * w).sum(-1))
        return twin.out[key].double().clone()

    best = value(digits)                                                                # every UAV staying
    for i in range(B):
        table[:, i, stay_d] = best
        choice = torch.full((N,), stay_d, dtype=torch.int64, device=env.device)
        for d in range(A - 1):
            digits[:, i] = d
            r = value(digits)
            table[:, i, d] = r
            win = (r > best) | (torch.isnan(best) & ~torch.isnan(r))                    # strict: stay, then the lowest digit, wins a tie
            best = torch.where(win, r, best)
            choice = torch.where(win, torch.full_like(choice, d), choice)
        digits[:, i] = choice
    return (digits * w).sum(-1), table, best
