"""Drop-in shim for the reference's `lpipsPyTorch` package: with `deblurgs_amd/dropin` on PYTHONPATH ahead of the
reference's own directory, test.py's and metrics.py's `from lpipsPyTorch import lpips` resolve to the MI355X operators
(dgs_lpips_alex, dgs_lpips_vgg, dgs_lpips_squeeze): all three backbones of the package.  The weights are those of
deblurgs_amd.lpips.set_default_weights(...), else the two files a user of torchvision and of the LPIPS package already has
under torch.hub.get_dir()/checkpoints (alexnet-owt-*.pth and alex.pth; vgg16-*.pth and vgg.pth; squeezenet1_1-*.pth and
squeeze.pth).  Only local files are opened: nothing is ever fetched.  See INTEGRATION.md."""
import torch

from deblurgs_amd import lpips as _lpips

# per backbone other than 'alex': torchvision's checkpoint, the LPIPS v0.1 linear layers, the weights class
_OPTIONAL = {'vgg': ("vgg16-*.pth", "vgg.pth", "LPIPSVggWeights"),
             'squeeze': ("squeezenet1_1-*.pth", "squeeze.pth", "LPIPSSqueezeWeights")}


def lpips(x: torch.Tensor, y: torch.Tensor, net_type: str = 'alex', version: str = '0.1'):
    """The reference's signature and result (lpipsPyTorch/__init__.py:6-21): [3,H,W] or [N,3,H,W] in, one [1,1,1,1]
    tensor out, summed over the layers and over the batch."""
    if net_type not in ('alex', 'vgg', 'squeeze'):
        raise NotImplementedError(f"choose net_type from [alex, squeeze, vgg] (got {net_type!r})")
    assert version in ['0.1'], 'v0.1 is only supported now'
    if net_type in _OPTIONAL:
        backbone, lin, cls = _OPTIONAL[net_type]
        try:
            w = _lpips.default_weights(x.device, net_type)
        except FileNotFoundError as e:
            raise NotImplementedError(
                f"deblurgs_amd evaluates LPIPS with the {net_type!r} backbone once its weights are there: torchvision's "
                f"{backbone} and the LPIPS v0.1 {lin} under torch.hub.get_dir()/checkpoints, or "
                f"deblurgs_amd.lpips.set_default_weights({cls}.load(backbone_path, lin_path)).  Without them only "
                "'alex' is evaluated.") from e
        return _lpips.lpips(x, y, w)
    return _lpips.lpips(x, y, _lpips.default_weights(x.device))
