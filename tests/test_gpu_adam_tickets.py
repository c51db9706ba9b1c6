"""FusedAdam's ticket words and graph capture: the words hgs_adam_step counts its workgroups in are created -- and zeroed --
BEFORE a capture (train.GraphedStep._make_capturable), never inside one.  Created lazily by the first captured step() they
lived in the graph pool and were zeroed by the single-step graph's replays alone; the several-steps graph, captured after it,
took its tickets from whatever that memory held when it was replayed first, and advanced no step counter."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_ticket_words_exist_before_the_capture_and_the_several_steps_graph_may_run_first(monkeypatch):
    from arguments import OptimizationParams
    from diff_gaussian_rasterization import _C as raster
    from hgs_runtime.fused import FusedAdam
    from synthetic import build_workload
    from train import GraphedStep
    created = []
    orig = FusedAdam.ticket_words

    def spy(self, dev):
        if self._tickets is None:
            created.append(torch.cuda.is_current_stream_capturing())
        return orig(self, dev)
    monkeypatch.setattr(FusedAdam, "ticket_words", spy)
    bg = torch.zeros(3, device="cuda")
    order = [1, 3, 0, 2]
    runs = {}
    try:
        for many_first in (True, False):
            model, cams, extent = build_workload("tiny", device="cuda", with_targets=True)
            opt = OptimizationParams()
            opt.enable_topology = False
            opt.inline_adam = False                      # Adam as a launch of its own: the one that takes tickets
            model.training_setup(opt)
            gs = GraphedStep(model, cams, opt, bg, extent=extent, steps_per_graph=4)
            gs.capture(cams)
            assert not gs.inline_adam and model.optimizer._tickets is not None
            if many_first:
                gs.step_many([cams[i] for i in order], 1)
            else:
                for k, i in enumerate(order):
                    gs.step(cams[i], 1 + k)
            gs.check()
            raster.set_async(False)
            state = []
            for g_ in model.optimizer.param_groups:
                p = g_["params"][0]
                st = model.optimizer.state.get(p, {})
                state += [p.detach().clone()] + [st[k].clone() for k in ("exp_avg", "exp_avg_sq", "step") if k in st]
            runs[many_first] = state
    finally:
        raster.set_async(False)
    assert created == [False, False]                     # one optimizer per run, its words made outside any capture
    for a, b in zip(runs[True], runs[False]):
        assert torch.equal(a, b)
    assert max(float(t) for t in runs[True] if t.ndim == 0) == 4.0
