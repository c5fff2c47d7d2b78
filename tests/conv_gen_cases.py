"""The geometries of the general matrix-core convolution (kernels/conv_gen.hip), shared by the plan test (no GPU) and the GPU test.

A case is (transposed, N, C_x, spatial, C_y, k, stride, pad, dil, output_padding): x is [N, C_x, *spatial], the weight [C_y, C_x, k...]
(transposed: [C_x, C_y, k...]); k, stride, pad, dil and output_padding are the same in both spatial dimensions of a 2-D case.

C5 has N = 65, not 64: with 64 images the weight gradient's K = 32768 divides evenly into the plan's splits on 256 compute units; the
test wants at least three splits with a ragged last one (65 images: 116 splits of 288, the last one 160).
"""

CASES = {
    "T1": (True, 2, 4, (5, 5), 3, 3, 2, 1, 1, 1),       # the existing tiny case; everything smaller than one tile
    "T2": (True, 3, 40, (8, 8), 24, 4, 2, 1, 1, 0),     # even filter; stride phases; K = 640; channels not multiples of 16
    "T3": (True, 2, 17, (7, 9), 33, 3, 1, 1, 2, 0),     # dilation; odd channels; non-square map; pixel tiles cross rows and images
    "T4": (True, 2, 20, (37,), 12, 5, 3, 2, 1, 2),      # 1-D transposed; stride 3 with output padding
    "T5": (True, 70, 16, (16, 16), 8, 3, 2, 1, 1, 1),   # many images; 8 output channels; weight-gradient K = 17920
    "C1": (False, 4, 32, (100,), 48, 3, 1, 1, 1, 0),    # the plain case
    "C2": (False, 1, 3, (1000,), 20, 7, 2, 3, 1, 0),    # K = 21 (below one bf16 k-step); N = 1; long rows
    "C3": (False, 5, 70, (33,), 130, 1, 1, 0, 1, 0),    # 1x1; 130 = 8 tiles + 2 columns
    "C4": (False, 2, 24, (64,), 24, 3, 1, 4, 4, 0),     # TCN dilation; padding wider than the filter
    "C5": (False, 65, 8, (512,), 24, 3, 1, 1, 1, 0),    # weight-gradient split-K, ragged last split (see above)
    "C6": (False, 3, 36, (50,), 20, 4, 3, 0, 2, 0),     # even filter with stride and dilation; no padding; remainder columns dropped
}


def regular_geometry(case):
    """(dims, taps) in the library's regular terms: dims = [N, Cin, H, W, Cout, Ho, Wo], taps = [kh, kw, sh, sw, ph, pw, dh, dw] (1-D: H = 1)"""
    transposed, N, cx, spatial, cy, k, s, p, d, op = case
    two = len(spatial) == 2

    def small(big):       # output extent of a regular convolution over `big`
        return (big + 2 * p - d * (k - 1) - 1) // s + 1

    def big(small_):      # output extent of the transposed one
        return (small_ - 1) * s - 2 * p + d * (k - 1) + op + 1

    if not transposed:
        cin, cout = cx, cy
        hw = list(spatial)
        howo = [small(v) for v in spatial]
    else:
        cin, cout = cy, cx
        howo = list(spatial)
        hw = [big(v) for v in spatial]
    if not two:
        hw, howo = [1] + hw, [1] + howo
    taps = [k if two else 1, k, s if two else 1, s, p if two else 0, p, d if two else 1, d]
    return [N, cin, hw[0], hw[1], cout, howo[0], howo[1]], taps
