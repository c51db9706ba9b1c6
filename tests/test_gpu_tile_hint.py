"""The loss head's tile hint (HgsHeadParams.tile_used) is in effect in the fused training step at the flagship frame size:
the SSIM backward's block lists leave out the blocks whose gradient nobody reads.  (Round 6 moved the hint 8 bytes off a
16-byte boundary at 1920 x 1080, the list builder dropped it without a word, and only the step time showed it.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lists_after_loss(fused, loss, H, W):
    # the head's scratch is one of the tensors the iteration saved for its backward; the block lists close it:
    # [n_work, n_zero_fill, -, -][work ids][zero-fill ids][12 spare words] (hgs_losses.hip head_block_lists)
    scratch = [t for t in loss.grad_fn.saved_tensors if t.dtype == torch.float32 and t.dim() == 1 and t.numel() > 9 * H * W]
    assert len(scratch) == 1
    s = scratch[0]
    nbs = 3 * ((H + 31) // 32) * ((W + 31) // 32)
    lists = s.view(torch.int32)[s.numel() - (2 * nbs + 16):].cpu()
    return int(lists[0]), int(lists[1]), nbs


@pytest.mark.parametrize("workload", ["north_star"])
def test_tile_hint_is_on_in_the_fused_step(workload):
    from arguments import OptimizationParams
    from hgs_runtime.strand_step import FusedStrandStep
    from synthetic import build_workload
    from utils.general import safe_state
    safe_state(True)
    model, cams, _ = build_workload(workload, device="cuda", with_targets=True, n_views=2)
    opt = OptimizationParams()
    model.training_setup(opt)
    fused = FusedStrandStep(model, cams, opt, torch.zeros(3, device="cuda"))
    H, W = cams[0].image_height, cams[0].image_width
    assert (W, H) == (1920, 1080)
    got = {}
    for skip in (False, True):
        fused.skip_unread_blocks = skip
        fused.views.select(1)
        loss, _ = fused.loss()
        got[skip] = _lists_after_loss(fused, loss, H, W)
        fused.backward(loss)
    torch.cuda.synchronize()
    (w0, z0, nbs), (w1, z1, _) = got[False], got[True]
    assert w0 + z0 == nbs                     # without the hint every block is filtered or zero-filled
    assert w1 + z1 < nbs                      # with it, the blocks nobody reads are on neither list
    assert w1 < w0 and w1 < nbs
