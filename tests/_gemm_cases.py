"""Shapes and reference arithmetic shared by the dense GEMM tests
(test_gpu_gemm.py, test_gpu_wgrad.py) and by test_gemm_cases_cpu.py, which
checks on the CPU that the cases cover what they claim to cover."""
import torch

# ---- mirrors of csrc/gemm_kernels.hip (tall_gemm_kernel and
# launch_tall_gemm); every threshold below is computed from these ----------
BM, BN, BK = 64, 64, 32   # C macro-tile and the k-stage
N_XCD = 8                 # the 1-D grid is dealt round-robin to 8 XCDs
WALK_BLOCKS = 4096        # launch_tall_gemm: walkers = 4096 / (8 * tn)

U = 2.0 ** -24            # fp32 unit roundoff
EXACT_LIMIT = 2 ** 24     # integers of magnitude <= 2^24 are exact in fp32


def n_tiles(n):
    return (n + BN - 1) // BN


def walkers_max(n):
    """Most m-walkers per (xcd, n-tile) that launch_tall_gemm ever uses."""
    return max(1, WALK_BLOCKS // (N_XCD * n_tiles(n)))


def m_stride_max(n):
    """Rows between two m-tiles of one block once M is large enough that
    the launcher uses every walker."""
    return N_XCD * walkers_max(n) * BM


def tiles_walked(m, n):
    """m-tiles walked by the busiest block for an [m, *] @ [*, n] call."""
    tm = (m + BM - 1) // BM
    per_xcd = (tm + N_XCD - 1) // N_XCD
    walkers = min(walkers_max(n), per_xcd)
    return (per_xcd + walkers - 1) // walkers


# ---- tall_gemm: small shapes ---------------------------------------------
GEMM_MS = (1, 63, 64, 65, 200)
GEMM_KS = (1, 4, 31, 32, 33, 47, 64, 100, 256)
GEMM_NS = (1, 5, 47, 64, 65, 100, 128, 130)

# pruned cross: every K with two (M, N), every N with two (M, K), every M
# with two (K, N), plus the two shapes the suite must always contain
GEMM_SMALL = sorted(set(
    [(65, k, 100) for k in GEMM_KS] + [(200, k, 5) for k in GEMM_KS]
    + [(63, 33, n) for n in GEMM_NS] + [(64, 64, n) for n in GEMM_NS]
    + [(m, 47, 130) for m in GEMM_MS] + [(m, 4, 64) for m in GEMM_MS]
    + [(65, 47, 47), (200, 256, 100), (1, 1, 1), (1, 256, 128)]))

# ---- tall_gemm: multi-tile walks -----------------------------------------
# A block takes a second m-tile only when M exceeds m_stride_max(N); the
# ragged "+ BM + 37" tail gives some blocks one tile more than others and
# ends on a partial tile.
_M_WALK3 = 2 * m_stride_max(512) + BM + 37   # N=512: tn=8, stride 32768
_M_WALK2 = m_stride_max(100) + BM + 37       # N=100: tn=2, stride 131072
GEMM_WALK = [
    (_M_WALK3, 8, 512),    # one k-stage: every iteration prefetches a tile
    (_M_WALK3, 40, 512),   # ragged second stage
    (_M_WALK3, 64, 512),   # exactly two stages
    (_M_WALK2, 72, 100),   # the routed data-grad shape
    (_M_WALK2, 256, 100),
]

# ---- wgrad ---------------------------------------------------------------
WGRAD_KS = (1, 31, 32, 33, 64, 65, 1000, 4099)
WGRAD_MNS = ((1, 1), (3, 5), (63, 65), (64, 64), (65, 63), (100, 47),
             (47, 100), (130, 256), (256, 130))
WGRAD_SMALL = sorted(set(
    [(k, 100, 47) for k in WGRAD_KS] + [(k, 63, 65) for k in WGRAD_KS]
    + [(33, m, n) for m, n in WGRAD_MNS]
    + [(1000, m, n) for m, n in WGRAD_MNS]
    + [(4099, 130, 256), (1, 1, 1)]))
# many chunks, a short last chunk and XCD padding blocks
WGRAD_FRONTIER = (200_001, 100, 256)


# ---- inputs and references -----------------------------------------------
def rand_ints(shape, bound, gen, device):
    """Integers in [-bound, bound], stored as fp32."""
    return torch.randint(-bound, bound + 1, shape, generator=gen,
                         device=device).float()


def gemm_bound(a, b, bias, k):
    """Elementwise fp64 error bound of ANY ordering of k fp32 fused
    multiply-adds plus one fp32 add: (k + 1) * 2^-24 * (|A| @ |B| + |bias|)."""
    mag = a.double().abs() @ b.double().abs()
    if bias is not None:
        mag = mag + bias.double().abs()
    return (k + 1) * U * mag
