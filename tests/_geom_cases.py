"""The cases shared by test_cvref_definition_host.py (oracle against the float64 definitions) and test_geometry_edges_gpu.py (kernels
against the oracle): shapes as ((H, W, C), (Wd, Hd)), plane sizes as (H, W), and the remap maps."""
import numpy as np

GPU_SUITE_F32 = [((30, 40, 3), (80, 60)), ((30, 40, 3), (40, 30)), ((33, 47, 3), (101, 77)), ((64, 80, 3), (20, 16)), ((50, 70, 3), (18, 12)),
                 ((50, 70, 3), (17, 13)), ((16, 20, 81), (80, 64)), ((12, 18, 1), (70, 50))]
GPU_SUITE_U8 = [((37, 49, 3), (64, 48)), ((48, 64, 3), (64, 48)), ((60, 84, 3), (1920, 1080)), ((5, 7, 3), (3, 2))]
EDGES = [((1, 1, 3), (5, 4)), ((1, 9, 2), (9, 3)), ((7, 1, 4), (1, 3)), ((2, 2, 5), (1, 1)), ((45, 64, 4), (48, 27)), ((270, 480, 4), (240, 135)),
         ((31, 1000, 3), (999, 30)), ((100, 100, 3), (99, 99)), ((3000, 7, 1), (7, 2999))]
SHAPES = GPU_SUITE_F32 + GPU_SUITE_U8 + EDGES
SOBEL_SIZES = [(37, 53), (1, 1), (1, 7), (6, 1), (2, 2), (3, 2)]
REMAP_SIZES = [(37, 53), (5, 4), (1, 1)]
NONFINITE = [np.nan, np.inf, -np.inf, 1e30, -1e30]


def spanning_maps(H, W, seed):
    """Float32 maps over the frame and 3 px beyond it on every side."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-3.0, W + 3.0, (H, W)).astype(np.float32), rng.uniform(-3.0, H + 3.0, (H, W)).astype(np.float32))


def put_nonfinite(mx, my):
    """NaN, +-inf and +-1e30 into the first elements of one map, then of the other (the partner coordinate stays inside the frame)."""
    mx, my = mx.copy(), my.copy()
    n = len(NONFINITE)
    fx, fy = mx.reshape(-1), my.reshape(-1)
    fx[:n], fy[:n] = NONFINITE, 0.25
    fy[n : 2 * n], fx[n : 2 * n] = NONFINITE, 0.25
    fx[2 * n], fy[2 * n] = np.nan, np.nan
    return mx, my
