"""The case table of krs_gemm_q8 (K18): one row per kernel and planner branch of keras_rs_amd/csrc/gemm_q8_plan.h, each the
smallest shape that reaches its branch.  tests/test_gemm_q8_host.py checks the table's coverage and every route without a
GPU (krs_gemm_q8_plan_route); tests/test_gemm_q8_gpu.py runs every row.

The ring keeps a chip-fill condition (at least 192 tiles of 256 x 256), so its rows are the smallest shapes that meet it:
about 49 152 x 256 outputs with K of a few pieces -- a few ms of int8 work each."""

from dataclasses import dataclass

KERNELS = ("generic", "tile128", "ring")
# why the planner chose the kernel: every branch of plan_gemm_q8
BRANCHES = (
    "ring",                  # every ring condition holds
    "tile:small_m",          # m < 256
    "tile:small_n",          # n < 256
    "tile:k_not_pieces",     # k is not whole 128-k pieces
    "tile:short_k",          # fewer than three pieces
    "tile:below_fill",       # fewer than 192 tiles of 256 x 256
    "generic:k",             # k is not a multiple of 16
    "generic:lda",           # lda is not a multiple of 16
    "generic:ldw",           # ldw is not a multiple of 16
    "generic:a_base",        # aq is not on 16 bytes
    "generic:w_base",        # wq is not on 16 bytes
)


@dataclass(frozen=True)
class Case:
    name: str
    m: int
    n: int
    k: int
    kernel: str
    branch: str
    k_tail: bool = False     # tile128 only: K is not whole 128-byte tile rows
    lda: int = 0             # 0: k
    ldw: int = 0             # 0: k
    ldc: int = 0             # 0: n
    a_off: int = 0           # byte offset of aq from a 16-byte boundary
    w_off: int = 0
    c_off: int = 0           # element offset of C from a 16-byte boundary

    def lds(self):
        return self.lda or self.k, self.ldw or self.k, self.ldc or self.n


FILL_M = 192 * 256           # 192 tiles against one tile of N

CASES = (
    # ---- generic: byte loads, one output per thread ----
    # K = 1, N and M odd: the shortest contraction there is
    Case("g_k1", 5, 7, 1, "generic", "generic:k"),
    # M = 1 with K = 13: the first bottom-MLP layer's contraction (13 dense features)
    Case("g_m1_k13", 1, 40, 13, "generic", "generic:k"),
    # K = 13 over more than one workgroup of outputs (130 x 512 = 260 workgroups)
    Case("g_k13", 130, 512, 13, "generic", "generic:k"),
    # K = 17: one more than the smallest tile-eligible K
    Case("g_k17", 33, 9, 17, "generic", "generic:k"),
    # aligned K but an lda that breaks 16-byte row alignment
    Case("g_lda", 33, 24, 32, "generic", "generic:lda", lda=40),
    # the same for the weight
    Case("g_ldw", 33, 24, 32, "generic", "generic:ldw", ldw=40),
    # aligned strides, base pointers off by 4 / 8 bytes
    Case("g_a_base", 20, 16, 32, "generic", "generic:a_base", a_off=4),
    Case("g_w_base", 20, 16, 32, "generic", "generic:w_base", w_off=8),
    # ---- 128 x 128 tiles ----
    # K = 16, the smallest tile-eligible K (one 16-byte chunk, the other seven zero-filled); one tile minus one row and column
    Case("t_k16_minus1", 127, 127, 16, "tile128", "tile:small_m", k_tail=True),
    # one tile plus one row and column (four workgroups, three of them one row or column wide), K one whole tile row
    Case("t_plus1", 129, 129, 128, "tile128", "tile:small_m"),
    # three tiles plus a ragged edge in both dimensions, K with a tail that is no multiple of 32 (48 = 32 + 16): the last
    # MFMA step is half zeros; N a multiple of 8 with every operand aligned, so the epilogue takes its vector path
    Case("t_three_ragged", 3 * 128 + 5, 3 * 128 + 8, 48, "tile128", "tile:k_not_pieces", k_tail=True),
    # one whole tile row of K plus a 16-byte tail: two K tiles, the second almost empty
    Case("t_k144", 64, 64, 144, "tile128", "tile:small_m", k_tail=True),
    # N = 1 (the last top-MLP layer) with an aligned K: the tile kernel with one live column
    Case("t_n1", 300, 1, 512, "tile128", "tile:small_n"),
    # M = 1 against a wide aligned weight
    Case("t_m1", 1, 264, 256, "tile128", "tile:small_m"),
    # padded leading dimensions on all three operands and an output base off by 4 elements (scalar epilogue)
    Case("t_padded", 130, 72, 160, "tile128", "tile:small_m", k_tail=True, lda=176, ldw=192, ldc=80, c_off=4),
    # K = 3456, the widest layer of the served model, at a few rows: the test data hold a row of -128 (one element 1) against a
    # column of 127, idot = -56 164 353 -- beyond 2^24 and odd, so the device's int -> float conversion has to round
    Case("t_k3456", 40, 24, 3456, "tile128", "tile:small_m"),
    # ring-sized in M and N with K of only two pieces: the ring's prologue needs three
    Case("t_two_pieces", FILL_M, 256, 256, "tile128", "tile:short_k"),
    # ring-sized, K = three pieces plus 16: not whole pieces
    Case("t_k400", FILL_M, 256, 400, "tile128", "tile:k_not_pieces", k_tail=True),
    # one tile short of the chip-fill bar (191 tiles)
    Case("t_below_fill", FILL_M - 256, 256, 384, "tile128", "tile:below_fill"),
    # ---- the ring ----
    # the smallest ring shape: exactly 192 tiles, K of exactly three pieces (prologue, no steady-state block, two tail blocks)
    Case("r_min", FILL_M, 256, 384, "ring", "ring"),
    # one more piece than that (one steady-state block); M one row short of 96 tiles, N one tile plus one column: clamped
    # DMA rows in both operands, a scalar epilogue (N = 257)
    Case("r_ragged", 96 * 256 - 1, 257, 512, "ring", "ring"),
    # three N tiles plus a ragged edge of 8 columns (four N tiles x 48 M tiles, the last M tile 3 rows tall), five pieces
    # (three steady-state blocks: every ring slot is reused), vector epilogue
    Case("r_three_tiles", 47 * 256 + 3, 3 * 256 + 8, 640, "ring", "ring"),
    # padded leading dimensions on the ring (rows are no longer back to back) and a padded output
    Case("r_padded", FILL_M, 256, 384, "ring", "ring", lda=400, ldw=416, ldc=264),
)

# epilogue forms every case runs (tests/test_gemm_q8_gpu.py): name -> operands present
FORMS = {
    "none": (),
    "bias": ("bias",),
    "cross": ("bias", "x0"),
    "cross_u": ("bias", "x0", "u"),
    "residual": ("r",),
}
