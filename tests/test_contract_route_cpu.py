"""ops.WeightView and ops.contract_route (no GPU).  A wrong stride triple still computes something, from the wrong
weights, and a wrong route still computes the right numbers on a slower kernel: the views are checked element by element
against plain torch indexing, and the routes of the product configuration, of the feature-pyramid variant and of the
discriminators are written out."""
import itertools

import pytest
import torch

MODES = ("fp32", "bf16x3", "bf16")
# the product configuration (oracle.crnn_oracle.CRNN_KWARGS): filters and map width of the seven blocks
FILTERS = [16, 32, 64, 128, 128, 128, 128]
WIDTHS = [128, 64, 32, 16, 8, 4, 2]
# (CIN, N, W, taps) of every forward contraction that goes through ops.contract; the first block (one input channel) is
# ops.block0_* / conv0_*, not a contraction of this table
BLOCKS = [(FILTERS[i - 1], FILTERS[i], WIDTHS[i], 9) for i in range(1, 7)]
FPN_LEVEL = (128, 128, 1, 3)                    # CRNN_fpn's pyramid levels: the 3x1 centre-column stencil
GRU_PROJECTIONS = [(128, 768, 1, 1), (256, 768, 1, 1)]
FUSE = (512, 256, 1, 1)                         # CRNN_fpn.conv1x1_2 / conv1x1_4
DENSE_SOFTMAX = (128, 128, 1, 1)                # CRNN_pred
FRAME_D = [(256, 128, 1, 1), (128, 32, 1, 1)]   # Frame_Discriminator.dense_d_1 / dense_d_2
S2D = [(512, 64, 64, 4), (256, 32, 32, 4)]      # Clip_Discriminator layers 2, 3 in space-to-depth form (4 * cin, co)
OTHERS = [FPN_LEVEL] + GRU_PROJECTIONS + [FUSE, DENSE_SOFTMAX] + FRAME_D + S2D


def _gather(wv):
    """(taps, K, N) tensor read through the view's offset and strides"""
    t, k, n = torch.meshgrid(torch.arange(len(wv.taps)), torch.arange(wv.K), torch.arange(wv.N), indexing="ij")
    return wv.tensor.reshape(-1)[wv.offset + t * wv.s_tap + k * wv.s_k + n * wv.s_n]


def _assert_dgrad(wv):
    """.dgrad(): the same weight element for (tap, k, n) -> (tap, n, k), at the negated tap offsets"""
    d = wv.dgrad()
    assert (d.K, d.N, d.offset, d.tensor is wv.tensor) == (wv.N, wv.K, wv.offset, True)
    assert list(d.taps) == [(-a, -b) for a, b in wv.taps]
    assert torch.equal(_gather(d), _gather(wv).permute(0, 2, 1))
    assert d.dgrad() == wv


@pytest.mark.parametrize("W", [16, 1])
def test_conv3x3_view_reads_the_torch_layout(W):
    from bsed_amd import ops
    co, cin = 5, 3
    w = torch.randn(co, cin, 3, 3, generator=torch.Generator().manual_seed(W))
    wv = ops.conv3x3_weight(w, W)
    assert (wv.K, wv.N) == (cin, co)
    got = _gather(wv)
    if W > 1:
        assert list(wv.taps) == [(t // 3 - 1, t % 3 - 1) for t in range(9)] == list(ops.TAPS3x3)
        for t in range(9):                                   # tap t of the nine-tap view is w[n, k, t // 3, t % 3]
            assert torch.equal(got[t], w[:, :, t // 3, t % 3].t())
    else:
        assert list(wv.taps) == [(-1, 0), (0, 0), (1, 0)] and (wv.offset, wv.s_tap) == (1, 3)
        for t in range(3):                                   # the centre column: w[n, k, t, 1]
            assert torch.equal(got[t], w[:, :, t, 1].t())
    assert torch.equal(_gather(wv._replace(tensor=wv.source(), offset=0)), got)   # what the pack kernels are handed
    _assert_dgrad(wv)
    grad = torch.randn(co, cin, 3, 3)
    gv = wv.over(grad)
    assert gv.tensor is grad and gv[1:] == wv[1:]


def test_linear_views_read_a_matrix_and_a_flat_slice():
    from bsed_amd import ops
    g = torch.Generator().manual_seed(3)
    w = torch.randn(6, 4, generator=g)                       # (N, K)
    wv = ops.linear_weight(w)
    assert (wv.K, wv.N, wv.offset, list(wv.taps)) == (4, 6, 0, [(0, 0)])
    assert torch.equal(_gather(wv)[0], w.t())
    _assert_dgrad(wv)
    # the GRU's double-direction input weights: a (2 * 3H, nin) matrix as a flat slice of the parameter arena
    arena, off, H3, nin = torch.randn(500, generator=g), 37, 12, 7
    flat = arena[off:off + 2 * H3 * nin]
    fv = ops.linear_weight(flat, 2 * H3, nin)
    assert torch.equal(_gather(fv)[0], flat.view(2 * H3, nin).t())
    assert fv.source() is flat
    _assert_dgrad(fv)
    # a (N, K, 1, 1) convolution weight with N and K given
    c = torch.randn(6, 4, 1, 1, generator=g)
    assert torch.equal(_gather(ops.linear_weight(c, 6, 4))[0], c.view(6, 4).t())


def test_plain_constructor_covers_the_other_layouts():
    from bsed_amd import ops
    g = torch.Generator().manual_seed(4)
    # direction dr's (3H, H) half of the recurrent weight gradient, its one tap a time shift
    H, ghh = 4, torch.randn(2, 12, 4, generator=g)
    for dr, shift in ((0, -1), (1, 1)):
        gv = ops.WeightView(ghh.view(-1), dr * 3 * H * H, ((shift, 0),), H, 3 * H, 0, 1, H)
        assert torch.equal(_gather(gv)[0], ghh[dr].t())
    # a (taps, K, N) weight, taps outermost: the discriminator's space-to-depth form
    full = torch.randn(4, 8, 3, generator=g)
    sv = ops.WeightView(full, 0, ((0, 0), (0, 1), (1, 0), (1, 1)), 8, 3, 8 * 3, 3, 1)
    assert torch.equal(_gather(sv), full)
    _assert_dgrad(sv)


def test_product_shapes_are_the_reference_configuration():
    from oracle import crnn_oracle as co
    assert list(co.CRNN_KWARGS["nb_filters"]) == FILTERS
    w, widths = 128, []
    for _, pw in co.CRNN_KWARGS["pooling"]:
        widths.append(w)
        w //= pw
    assert widths == WIDTHS and w == 1


@pytest.mark.parametrize("mode", MODES)
def test_routes_of_the_product_configuration_the_fpn_variant_and_the_discriminators(mode):
    from bsed_amd import ops
    assert ops.igemm3s_supported(64, 16) and ops.igemm3s_supported(64, 32)
    fwd = [ops.contract_route("forward", cin, n, W, taps, mode) for cin, n, W, taps in BLOCKS + OTHERS]
    # a data gradient contracts over the layer's output channels
    dgrad = [ops.contract_route("dgrad", n, cin, W, taps, mode) for cin, n, W, taps in BLOCKS + OTHERS]
    if mode == "fp32":
        assert fwd == dgrad == ["igemm"] * (len(BLOCKS) + len(OTHERS))
    else:   # the 16 -> 32 block both ways: its weight table stays in LDS; everything else has CIN a multiple of 32
        assert fwd == dgrad == ["igemm3s"] + ["igemm3"] * (len(BLOCKS) - 1 + len(OTHERS))


@pytest.mark.parametrize("mode", MODES)
def test_shapes_the_bf16_core_kernels_are_not_built_for(mode):
    from bsed_amd import ops
    # three taps, CIN not a multiple of 32: the width-1 stencil of a 16-channel input
    assert ops.contract_route("forward", 16, 32, 1, 3, mode) == "igemm"
    # the LDS-resident kernel is a nine-tap kernel: a 1-tap contraction with its channel counts is not its business
    assert ops.contract_route("forward", 16, 32, 64, 1, mode) == "igemm"
    assert ops.contract_route("dgrad", 32, 16, 64, 1, mode) == ("igemm" if mode == "fp32" else "igemm3")
    # ... and it holds the patch of one tile: not on a map as wide as the first block's
    assert not ops.igemm3s_supported(1, 16) and not ops.igemm3s_supported(1, 32)
    assert ops.contract_route("forward", 16, 32, 1, 9, mode) == "igemm"
    # the dgrad form is the 32 -> (at most 32) one; forward 32 -> 64 and dgrad 32 -> 64 are igemm3's
    assert ops.contract_route("forward", 32, 64, 64, 9, mode) == ("igemm" if mode == "fp32" else "igemm3")
    assert ops.contract_route("dgrad", 32, 64, 64, 9, mode) == ("igemm" if mode == "fp32" else "igemm3")
    assert ops.contract_route("dgrad", 32, 32, 64, 9, mode) == ("igemm" if mode == "fp32" else "igemm3s")


def test_unknown_mode_or_direction_is_refused():
    from bsed_amd import ops
    from bsed_amd._lib import BsedError
    for direction, mode in itertools.product(("forward", "dgrad"), ("fp16", None)):
        with pytest.raises(BsedError, match=repr(mode)):
            ops.contract_route(direction, 32, 64, 64, 9, mode)
    with pytest.raises(BsedError, match="backward"):
        ops.contract_route("backward", 32, 64, 64, 9, "fp32")
