"""In-test oracle of the compact generator: a float64 CPU restatement of upstream Real-ESRGAN's SRVGGNetCompact
(nn.Conv2d + nn.PReLU / LeakyReLU(0.1) / ReLU, pixel_shuffle, nearest-upsampled residual).  Own code: the reference project
has no such model."""
import torch
import torch.nn.functional as F
from torch import nn


class UpstreamCompact(nn.Module):
    """The upstream module tree (body = ModuleList of conv / activation, upsampler = PixelShuffle): state_dict keys and init."""

    def __init__(self, num_conv=16, upscale=4, act_type="prelu"):
        super().__init__()
        self.body = nn.ModuleList()
        self.body.append(nn.Conv2d(3, 64, 3, 1, 1))
        self.body.append(self._act(act_type))
        for _ in range(num_conv):
            self.body.append(nn.Conv2d(64, 64, 3, 1, 1))
            self.body.append(self._act(act_type))
        self.body.append(nn.Conv2d(64, 3 * upscale * upscale, 3, 1, 1))
        self.upsampler = nn.PixelShuffle(upscale)

    @staticmethod
    def _act(act_type):
        return {"prelu": lambda: nn.PReLU(num_parameters=64), "leakyrelu": lambda: nn.LeakyReLU(0.1, True),
                "relu": lambda: nn.ReLU(True)}[act_type]()


def compact_forward64(x, sd, num_conv, upscale, act_type):
    """float64 forward of upstream's SRVGGNetCompact on the CPU."""
    h = x.double().cpu()
    for k in range(num_conv + 1):
        h = F.conv2d(h, sd[f"body.{2 * k}.weight"].double().cpu(), sd[f"body.{2 * k}.bias"].double().cpu(), padding=1)
        if act_type == "prelu":
            h = F.prelu(h, sd[f"body.{2 * k + 1}.weight"].double().cpu())
        elif act_type == "leakyrelu":
            h = F.leaky_relu(h, 0.1)
        else:
            h = F.relu(h)
    last = 2 * (num_conv + 1)
    h = F.conv2d(h, sd[f"body.{last}.weight"].double().cpu(), sd[f"body.{last}.bias"].double().cpu(), padding=1)
    return F.pixel_shuffle(h, upscale) + F.interpolate(x.double().cpu(), scale_factor=upscale, mode="nearest")
