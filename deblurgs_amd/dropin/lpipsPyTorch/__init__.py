"""Drop-in shim for the reference's `lpipsPyTorch` package: with `deblurgs_amd/dropin` on PYTHONPATH ahead of the
reference's own directory, test.py's `from lpipsPyTorch import lpips` resolves to the MI355X operator (dgs_lpips_alex).
The weights are those of deblurgs_amd.lpips.set_default_weights(...), else the two files a user of torchvision and of the
LPIPS package already has under torch.hub.get_dir()/checkpoints (alexnet-owt-*.pth, alex.pth).  Only local files are
opened: nothing is ever fetched.  See INTEGRATION.md."""
import torch

from deblurgs_amd import lpips as _lpips


def lpips(x: torch.Tensor, y: torch.Tensor, net_type: str = 'alex', version: str = '0.1'):
    """The reference's signature and result (lpipsPyTorch/__init__.py:6-21): [3,H,W] or [N,3,H,W] in, one [1,1,1,1]
    tensor out, summed over the layers and over the batch."""
    if net_type != 'alex':
        raise NotImplementedError(f"deblurgs_amd implements LPIPS with the 'alex' backbone only (got {net_type!r})")
    assert version in ['0.1'], 'v0.1 is only supported now'
    return _lpips.lpips(x, y, _lpips.default_weights(x.device))
