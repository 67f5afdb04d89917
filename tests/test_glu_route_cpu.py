"""ops.glu_route (no GPU): which kernel route runs the GLU half of a CNN block.  A wrong branch still computes the right
numbers on a slower kernel, which no numeric test sees; the table below is the routes of the product configuration, of
the feature-pyramid level and of the shapes where a kernel is not built, written out."""
import itertools

import pytest

MODES = ("fp32", "bf16x3", "bf16")
# the product configuration (oracle.crnn_oracle.CRNN_KWARGS): filters, pooling window and map width of the seven blocks
FILTERS = [16, 32, 64, 128, 128, 128, 128]
POOLING = [(2, 2), (2, 2)] + [(1, 2)] * 5
WIDTHS = [128, 64, 32, 16, 8, 4, 2]
FPN_LEVEL = (128, 1, (2, 1))      # CRNN_fpn's pyramid levels: C, W, pool
SHAPES = list(zip(FILTERS, WIDTHS, POOLING)) + [FPN_LEVEL]

# {(mode is fp32): routes of the eight shapes above}
FORWARD = {True: ["glu16"] + ["igemm"] * 7,
           False: ["glu16"] + ["glu3"] * 7}
BACKWARD_FUSED = {True: ["glu16"] + ["fused_fp32"] * 7,
                  False: ["glu16", "glu3", "glu3"] + ["glu3n"] * 5}
BACKWARD_UNFUSED = ["glu16"] + ["unfused"] * 7


def test_product_shapes_are_the_reference_configuration():
    from oracle import crnn_oracle as co
    assert list(co.CRNN_KWARGS["nb_filters"]) == FILTERS
    assert [tuple(p) for p in co.CRNN_KWARGS["pooling"]] == POOLING
    w, widths = 128, []
    for _, pw in POOLING:
        widths.append(w)
        w //= pw
    assert widths == WIDTHS and w == 1


@pytest.mark.parametrize("mode,fused", list(itertools.product(MODES, (True, False))))
def test_routes_of_the_product_configuration_and_the_fpn_level(mode, fused):
    from bsed_amd import ops
    fwd = [ops.glu_route("forward", C, W, pool, mode, fused) for C, W, pool in SHAPES]
    bwd = [ops.glu_route("backward", C, W, pool, mode, fused) for C, W, pool in SHAPES]
    assert fwd == FORWARD[mode == "fp32"]                    # `fused` is a switch of the backward only
    assert bwd == (BACKWARD_FUSED[mode == "fp32"] if fused else BACKWARD_UNFUSED)
    assert ops.glu_route("forward", 32, 64, (2, 2), mode) == fwd[1]      # fused defaults to True


@pytest.mark.parametrize("mode", MODES)
def test_forward_falls_to_igemm_where_the_bf16_core_kernel_is_not_built(mode):
    """C = 32 on a width-4 map with a (2, 2) pool: the tile is 32 x 4, a width the pooled store of glu_fwd3 has no form for"""
    from bsed_amd import ops
    assert ops.tile_for(4) == (32, 4) and not ops.glu_fwd3_supported(4, 32, (2, 2))
    assert ops.glu_route("forward", 32, 4, (2, 2), mode) == "igemm"
    assert ops.glu_route("backward", 32, 4, (2, 2), mode) == ("fused_fp32" if mode == "fp32" else "glu3")


def test_unknown_mode_or_direction_is_refused():
    from bsed_amd import ops
    from bsed_amd._lib import BsedError
    with pytest.raises(BsedError, match="fp16"):
        ops.glu_route("forward", 32, 64, (2, 2), "fp16")
    with pytest.raises(BsedError, match="fp16"):
        ops.glu_route("backward", 16, 128, (2, 2), "fp16", False)
    with pytest.raises(BsedError, match="sideways"):
        ops.glu_route("sideways", 32, 64, (2, 2), "fp32")
