"""engine/capture.py's `capture_graph`, and the one roll-back rule across a
real capture: a stepped torch Adam keeps its state."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_capture_graph_warms_up_rolls_back_and_records():
    from esr_amd.engine.capture import capture_graph
    c = torch.zeros(1, device=DEV)

    def body():
        c.add_(1)
        return c * 2

    graph, out = capture_graph(body, warmup=2,
                               after_warmup=lambda: c.zero_())
    # warm-up ran and was undone; capture recorded, it did not run
    assert c.item() == 0
    graph.replay()
    assert c.item() == 1 and out.item() == 2
    graph.replay()
    graph.replay()
    assert c.item() == 3 and out.item() == 6

    # a second graph out of the first one's memory pool
    d = torch.zeros(1, device=DEV)

    def body2():
        d.add_(c)
        return d + 1

    graph2, out2 = capture_graph(body2, warmup=2, pool=graph.pool(),
                                 after_warmup=lambda: d.zero_())
    assert d.item() == 0
    graph2.replay()
    assert d.item() == 3 and out2.item() == 4
    graph.replay()
    graph2.replay()
    assert c.item() == 4 and d.item() == 7 and out2.item() == 8


def test_stepped_adam_survives_capture():
    """Adam stepped twice before capture() (a run resumed from a checkpoint
    brings such state): the warm-up roll-back hands parameters, moments and
    step back bit for bit, and the first replay is step 3."""
    from esr_amd.engine.graph_runner import GraphedBPTTStep, flatten_grads
    from esr_amd.models import build_model

    device = torch.device(DEV)
    torch.manual_seed(0)
    model = build_model("ESRNet", inch=2, basech=8, num_frame=3,
                        upsampler="pixelshuffle").to(device)
    params = [p for p in model.parameters() if p.requires_grad]
    flat = flatten_grads(params, device)
    opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
    for _ in range(2):
        flat.copy_(torch.randn_like(flat) * 1e-3)
        opt.step()
    torch.cuda.synchronize()

    def everything():
        out = [p.detach() for p in params]
        for p in params:
            s = opt.state[p]
            out += [s["exp_avg"], s["exp_avg_sq"], s["step"]]
        return out

    before = [t.clone() for t in everything()]
    assert all(float(opt.state[p]["step"]) == 2 for p in params)

    runner = GraphedBPTTStep(
        model, opt, flat, n_windows=2, inp_shape=(2, 4, 2, 32, 32),
        gt_shape=(2, 2, 2, 32, 32), device=device,
        amp_dtype=torch.bfloat16, sequence=True, seqn=3)
    runner.capture()
    for now, then in zip(everything(), before):
        assert torch.equal(now, then), "capture() changed a resumed run"

    x = torch.randn(2, 4, 2, 32, 32, device=device)
    g = torch.randn(2, 2, 2, 32, 32, device=device)
    loss, _ = runner.run([x], [g])
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert all(float(opt.state[p]["step"]) == 3 for p in params)
    assert any(not torch.equal(p.detach(), b) for p, b in zip(params, before))
