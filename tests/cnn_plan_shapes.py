"""The shapes at which tests/test_cnn_plans_gpu.py compares libuavcnn.so's kernels with float64 PyTorch, in one place:
tests/test_cnn_agent.py::test_plan_shapes_select_their_branches asks the library's own launch plans (the host-only
uavcnn_*_workspace_bytes functions) whether the *_DEEP / *_MULTI shapes still reach the branch they are here for, so a change of a plan
cannot quietly turn the GPU cases back into single-chunk / single-sample ones.  No GPU, no torch: importable anywhere."""

# dense_fwd: (M, D) whose plan gives every slice more than one 64-chunk, so dense_fwd_kernel's k0 loop restages wl at least twice
DENSE_DEEP = [(130, 44805), (1100, 20000), (3, 353440)]
# ... and the flatten of G = 13 (D < 16: one partial tile in every dense kernel)
DENSE_SHAPES = DENSE_DEEP + [(2, 10)]

# conv1 forward / weight gradient at K > 64 (nodes in wavefronts 1..3): G, M and (n_bs, K); M samples on fewer workgroups than samples
CONV1_MULTI_G, CONV1_MULTI_M = 17, 1030
CONV1_MULTI_NBS_K = [(16, 256), (16, 65), (1, 129)]
# conv1 at the grid limits the API accepts: (G, M, n_bs, K)
CONV1_LIMITS = [(13, 5, 4, 44), (200, 2, 16, 216)]

# conv5 forward, dX and weight gradient: (S, M).  CONV5_MULTI: more (sample, row) pairs than conv5_wgrad workgroups
CONV5_MULTI = [(5, 1500)]
CONV5_SHAPES = CONV5_MULTI + [(9, 3), (196, 2)]
