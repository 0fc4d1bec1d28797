"""The test-view pose fit driven through render(), torch.autograd and torch.optim.Adam: the yardstick
deblurgs_amd.evaluation.FusedPoseFit is tested (tests/test_gpu_evaluation.py) and timed (tools/eval_timing.py) against.
Test infrastructure, not part of the package."""
import torch

from deblurgs_amd import evaluation as ev, gaussian_renderer


class AutogradPoseFit:
    """The same fit driven through render(), torch.autograd and torch.optim.Adam, statement for statement what
    test.py:145-180 runs (one blocking read of the duplicate count and of the MSE per step, a full backward into every
    per-Gaussian parameter that is then thrown away): the yardstick FusedPoseFit is tested and timed against."""

    def __init__(self, cloud, cams, gt_images, bg, tone_mapping, num_iter_per_view=2000, model=None):
        self.cloud, self.bg = cloud, bg
        self.model = model if model is not None else ev.TestPoseModel(cams, device=cloud._xyz.device)
        self.gt = [g.to(cloud._xyz.device, torch.float32) for g in gt_images]
        self.tone_mapping = ev._tone_args(tone_mapping)[0]
        self.optimizer = torch.optim.Adam([{"params": [self.model._rot], "lr": ev.ROT_LR, "name": "rot"},
                                           {"params": [self.model._trans], "lr": ev.TRANS_LR, "name": "trans"}],
                                          lr=ev.TRANS_LR, eps=ev.ADAM_EPS)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=max(int(num_iter_per_view) // ev.LR_STAGES, 1),
                                                         gamma=ev.LR_GAMMA)
        self.l2_error_ema = 0.0

    def step(self, idx):
        cam = self.model(idx)
        image = gaussian_renderer.render(cam, self.cloud, self.bg)["render"]
        loss, mse = ev.view_loss(image, self.gt[idx], self.tone_mapping)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        self.l2_error_ema = self.l2_error_ema * 0.6 + mse.item() * 0.4
        return loss.detach()

    def run(self, orders):
        for order in orders:
            for idx in order:
                self.step(idx)
            self.scheduler.step()
