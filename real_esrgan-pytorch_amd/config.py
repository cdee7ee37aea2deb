"""Configuration with the reference's names and values (reference config.py:20-158).

Differences, all additive: `device` follows the visible GPU instead of hard-coding cuda:0 when
LOCAL_RANK is set (one process per GPU), `precision` selects the kernel arithmetic, and the
cudnn.benchmark switch is dropped (no cuDNN / MIOpen on this path).  `mode` gates the same
name groups as the reference.
"""
import os
import random

import numpy as np
import torch

degradation_model_parameters_dict = {
    "sinc_kernel_size": 21,
    "gaussian_kernel_range": [7, 9, 11, 13, 15, 17, 19, 21],
    "gaussian_kernel_type": ["isotropic", "anisotropic",
                             "generalized_isotropic", "generalized_anisotropic",
                             "plateau_isotropic", "plateau_anisotropic"],
    "gaussian_kernel_probability1": [0.45, 0.25, 0.12, 0.03, 0.12, 0.03],
    "sinc_kernel_probability1": 0.1,
    "gaussian_sigma_range1": [0.2, 3],
    "generalized_kernel_beta_range1": [0.5, 4],
    "plateau_kernel_beta_range1": [1, 2],
    "gaussian_kernel_probability2": [0.45, 0.25, 0.12, 0.03, 0.12, 0.03],
    "sinc_kernel_probability2": 0.1,
    "gaussian_sigma_range2": [0.2, 1.5],
    "generalized_kernel_beta_range2": [0.5, 4],
    "plateau_kernel_beta_range2": [1, 2],
    "sinc_kernel_probability3": 0.8,
}

degradation_process_parameters_dict = {
    "first_blur_probability": 1.0,
    "resize_probability1": [0.2, 0.7, 0.1],
    "resize_range1": [0.15, 1.5],
    "gray_noise_probability1": 0.4,
    "gaussian_noise_probability1": 0.5,
    "noise_range1": [1, 30],
    "poisson_scale_range1": [0.05, 3],
    "jpeg_range1": [30, 95],
    "second_blur_probability": 0.8,
    "resize_probability2": [0.3, 0.4, 0.3],
    "resize_range2": [0.3, 1.2],
    "gray_noise_probability2": 0.4,
    "gaussian_noise_probability2": 0.5,
    "noise_range2": [1, 25],
    "poisson_scale_range2": [0.05, 2.5],
    "jpeg_range2": [30, 95],
}

# Random seed to maintain reproducible results (reference config.py:64-66)
random.seed(0)
torch.manual_seed(0)
np.random.seed(0)
device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
# Kernel arithmetic, following the reference's own call sites:
#   train / validate run under amp.autocast (train_realesrnet.py:383,461; train_realesrgan.py:471,...)  ->  `precision`, default
#     "fast" = f16 operands on the MFMA pipe, fp32 accumulation (the autocast numerics class);
#   inference.py:52-53 and test.py:79-80 run the generator in plain fp32 (no autocast)               ->  `inference_precision`,
#     default "exact16" = split-operand f16 MFMA, fp32-class results (the mode inside the 1e-3 parity tolerance).
# "strict" (f32 MFMA) is accepted by both; inference.py --precision, $RESR_PRECISION (train) and $RESR_INFERENCE_PRECISION override.
# Output parity ($RESR_OUTPUT_PARITY=1; off by default): outputs and losses inside the 1e-3 tolerance, gradients in fast mode's class.
# Precision exact16, the generator on x2_plan 2401 (_lib.X2_PLAN_OUTPUT_PARITY: the inference MX forward in training, an f16
# backward pass behind it), the discriminator and ContentLoss with f16_backward=True (exact16 forward, fast mode's backward pass).
# The train scripts take their module arguments from generator_options() / backward_options() below.
output_parity = os.environ.get("RESR_OUTPUT_PARITY", "0") == "1"
precision = os.environ.get("RESR_PRECISION", "exact16" if output_parity else "fast")
if output_parity and precision != "exact16":
    raise ValueError(f"RESR_OUTPUT_PARITY=1 runs in exact16; RESR_PRECISION={precision!r} contradicts it")
inference_precision = os.environ.get("RESR_INFERENCE_PRECISION", "exact16")
# Generator architecture of the train scripts, their validate() and test.py (build_generator() below): "rrdb" = `Generator`, the
# reference's RRDBNet; "compact" = `SRVGGNetCompact` (upstream's realesr-animevideov3 / realesr-general-x4v3 family) with
# `compact_num_conv` body convs and `compact_act_type` activations, trainable=True in the train scripts ("fast" or "strict").
g_arch = os.environ.get("RESR_G_ARCH", "rrdb")
if g_arch not in ("rrdb", "compact"):
    raise ValueError(f"RESR_G_ARCH={g_arch!r}: expected 'rrdb' or 'compact'")
if output_parity and g_arch == "compact":
    raise ValueError("RESR_OUTPUT_PARITY=1 runs in exact16; exact16 training of the compact generator (RESR_G_ARCH=compact) is not built")
compact_num_conv = int(os.environ.get("RESR_COMPACT_NUM_CONV", "16"))
compact_act_type = os.environ.get("RESR_COMPACT_ACT", "prelu")
# An upstream checkpoint ({"params_ema": sd} / {"params": sd} / a bare state dict: model.load_official_state_dict, RRDB or compact
# keys) loaded into the generator after build_model() and before any `resume*` is applied; "" = none.
pretrained_g = os.environ.get("RESR_PRETRAINED_G", "")
# Where the train scripts' training batches come from (their load_dataset(); validation and test are the loader's either way):
# "loader" = DataLoader workers + `dataset.CUDAPrefetcher`, the reference's host pipeline; "device" = `device_data.DeviceTileSource`,
# the training tiles resident in HBM as uint8, augmentation and blur-kernel synthesis as two launches per batch.
# "paired" / "paired_loader" = fine-tuning on LR / HR pairs of the user's own instead of pairs the degradation stage synthesises: the HR
# files in `train_image_dir`, their LR partners (same names, 1 / upscale_factor the size) in `paired_lr_image_dir` ($RESR_PAIRED_LR_DIR);
# "paired" = `device_data.PairedDeviceSource`, both sides resident in HBM as uint8 and a batch one launch; "paired_loader" =
# `dataset.PairedImageDataset` in DataLoader workers, the fallback for a set that does not fit.  The LR patch is paired_patch() below.
# "images" / "images_loader" = whole training images of any size in `train_image_dir`, no offline tiling: a sample is a random
# `train_tile` x `train_tile` window of its image, reflect-padded below / to the right where the image is smaller (upstream's
# crop_pad_size); "images" = `device_data.ImageCropSource`, the images resident in HBM as uint8 and the crop inside the batch's launch;
# "images_loader" = `dataset.CropImageDataset` in DataLoader workers, the fallback for a set that does not fit.
DATA_SOURCES = ("loader", "device", "paired", "paired_loader", "images", "images_loader")
PAIRED_DATA_SOURCES = ("paired", "paired_loader")
IMAGE_DATA_SOURCES = ("images", "images_loader")
data_source = os.environ.get("RESR_DATA_SOURCE", "loader")
if data_source not in DATA_SOURCES:
    raise ValueError(f"RESR_DATA_SOURCE={data_source!r}: expected one of " + ", ".join(repr(name) for name in DATA_SOURCES))
# The window side T of the two whole-image sources (upstream's crop_pad_size); the other sources never read it.
train_tile = int(os.environ.get("RESR_TRAIN_TILE", "400"))
# The multi-scale copies of the two whole-image sources (step 1 of upstream's data preparation, made at load instead of offline): every
# image also enters the set as its Pillow-LANCZOS copy at each of `train_scales` (RESR_TRAIN_SCALES: comma-separated, each a float or a/b,
# e.g. "0.75,0.5,1/3") and, with `train_short_side` = S > 0 (RESR_TRAIN_SHORT_SIDE, upstream: 400), as one more copy whose shorter side is
# S.  Empty / 0 = no copies, the sources as they were.  Parsed and checked by train_copies() below; the other sources never read them.
train_scales = os.environ.get("RESR_TRAIN_SCALES", "")
train_short_side = int(os.environ.get("RESR_TRAIN_SHORT_SIDE", "0"))
paired_lr_image_dir = os.environ.get("RESR_PAIRED_LR_DIR", "")
if data_source in PAIRED_DATA_SOURCES and not paired_lr_image_dir:
    raise ValueError(f"RESR_DATA_SOURCE={data_source!r} needs RESR_PAIRED_LR_DIR: the directory of the LR partners of the files in train_image_dir")
# The training pair pool of the train scripts (device_data.PairPool, attached by train_realesrnet.train_pairs behind every data source):
# 0 = off, the code as it was; Q > 0 = a resident queue of Q finished (lr, hr) pairs that each step's batch is exchanged with once it is
# full, so that a batch mixes samples of many degradation plans.  Upstream Real-ESRGAN trains with 180 (at 12 per GPU); in a training
# mode Q must be a multiple of batch_size (checked below, where batch_size is known).
pair_pool_size = int(os.environ.get("RESR_PAIR_POOL", "0"))
if pair_pool_size < 0:
    raise ValueError(f"RESR_PAIR_POOL={pair_pool_size}: expected 0 (off) or the number of pairs the pool holds")
niqe_model_path = "./results/pretrained_models/niqe_model.mat"
# How validate() and test.py compute NIQE (build_niqe() below): "torch" = `image_quality_assessment.NIQE`, plain torch in float64;
# "native" = `NativeNIQE`, the features by the kernels of csrc/niqe.hip (same tail, same prior; its luma is the kernels' stated fp32 order).
niqe_backend = os.environ.get("RESR_NIQE", "torch")
if niqe_backend not in ("torch", "native"):
    raise ValueError(f"RESR_NIQE={niqe_backend!r}: expected 'torch' or 'native'")
# The tail of the native score (features -> score): "torch" = the function `niqe()` uses, image by image; "native" = two launches for the
# whole batch (resr_niqe_score), no host round trip.  Only the native backend has a choice.
niqe_tail = os.environ.get("RESR_NIQE_TAIL", "torch")
if niqe_tail not in ("torch", "native"):
    raise ValueError(f"RESR_NIQE_TAIL={niqe_tail!r}: expected 'torch' or 'native'")
if niqe_tail == "native" and niqe_backend != "native":
    raise ValueError("RESR_NIQE_TAIL=native needs RESR_NIQE=native: the torch backend has no native tail")
# Whether validate() and test.py also score SR against its ground truth (build_full_ref() below): "off" = NIQE alone, the code as it
# was; "torch" = PSNR / SSIM of the Y channel in torch float64 (`image_quality_assessment.psnr` / `ssim`); "native" = `NativeFullRef`,
# both in one pass of csrc/fullref.hip.
full_ref = os.environ.get("RESR_FULL_REF", "off")
if full_ref not in ("off", "torch", "native"):
    raise ValueError(f"RESR_FULL_REF={full_ref!r}: expected 'off', 'torch' or 'native'")
# Which quantity build_full_ref()'s module scores: "y" = the BT.601 luma level (the code as it was); "rgb" = BasicSR's
# `test_y_channel: false`, the PSNR over all three channels and the mean of the per-channel SSIMs (`full_ref_channels*`), through the
# backend RESR_FULL_REF selects and under the same scalar names.
full_ref_channels = os.environ.get("RESR_FULL_REF_CHANNELS", "y")
if full_ref_channels not in ("y", "rgb"):
    raise ValueError(f"RESR_FULL_REF_CHANNELS={full_ref_channels!r}: expected 'y' or 'rgb'")
in_channels = 3
out_channels = 3
upscale_factor = 4
mode = os.environ.get("RESR_MODE", "train_realesrnet")
exp_name = "RealESRNet_baseline"

if mode == "train_realesrnet":
    train_image_dir = "./data/DIV2K/Real_ESRGAN/train"
    valid_image_dir = "./data/DIV2K/Real_ESRGAN/valid"
    test_lr_image_dir = f"./data/Set5/LRbicx{upscale_factor}"
    test_hr_image_dir = "./data/Set5/GTmod12"
    image_size = 256
    batch_size = 48
    num_workers = 4
    resume = ""
    epochs = 1298
    model_lr = 2e-4
    model_betas = (0.9, 0.99)
    ema_model_weight_decay = 0.999
    lr_scheduler_step_size = epochs // 5
    lr_scheduler_gamma = 0.5
    print_frequency = 200

if mode == "train_realesrgan":
    train_image_dir = "./data/DIV2K/Real_ESRGAN/train"
    valid_image_dir = "./data/DIV2K/Real_ESRGAN/valid"
    test_lr_image_dir = f"./data/Set5/LRbicx{upscale_factor}"
    test_hr_image_dir = "./data/Set5/GTmod12"
    image_size = 256
    batch_size = 48
    num_workers = 4
    resume = "./results/RealESRNet_baseline/g_last.pth.tar"
    resume_d = ""
    resume_g = ""
    epochs = 519
    feature_model_extractor_nodes = ["features.2", "features.7", "features.16", "features.25", "features.34"]
    feature_model_normalize_mean = [0.485, 0.456, 0.406]
    feature_model_normalize_std = [0.229, 0.224, 0.225]
    pixel_weight = 1.0
    content_weight = [0.1, 0.1, 1.0, 1.0, 1.0]
    adversarial_weight = 0.1
    model_lr = 1e-4
    model_betas = (0.9, 0.99)
    ema_model_weight_decay = 0.999
    lr_scheduler_milestones = [int(epochs * 0.125), int(epochs * 0.250), int(epochs * 0.500), int(epochs * 0.750)]
    lr_scheduler_gamma = 0.5
    print_frequency = 200

if mode == "test":
    lr_dir = f"./data/Set5/LRbicx{upscale_factor}"
    sr_dir = f"./results/test/{exp_name}"
    hr_dir = "./data/Set5/GTmod12"
    model_path = "./results/pretrained_models/RealESRGAN_x4-DFO2K-678bf481.pth.tar"


def paired_patch() -> int:
    """The LR patch side of the paired data sources: image_size // upscale_factor (image_size stays the HR crop, as in the other modes)."""
    if image_size < upscale_factor or image_size % upscale_factor:
        raise ValueError(f"config.image_size={image_size} is not a multiple of upscale_factor={upscale_factor}: the paired data sources "
                         "crop an LR patch of image_size // upscale_factor and its exact HR block")
    return image_size // upscale_factor


if data_source in PAIRED_DATA_SOURCES and mode in ("train_realesrnet", "train_realesrgan"):
    paired_patch()


def train_window() -> int:
    """The window side of the whole-image data sources: `train_tile`, which the degradation stage crops its image_size HR patch from."""
    if train_tile < image_size:
        raise ValueError(f"config.train_tile={train_tile} (RESR_TRAIN_TILE) is below image_size={image_size}: the whole-image data sources "
                         "hand out train_tile windows, and the HR crop of image_size is taken inside them")
    return train_tile


def check_train_copies(scales, short_side):
    """(scales as a tuple of floats, short_side as an int), or ValueError by name: a scale that is not finite or not in (0, 1) -- 1 would
    duplicate the image --, a negative short side."""
    import math
    try:
        scales = tuple(float(s) for s in scales)
    except (TypeError, ValueError):
        raise ValueError(f"train_scales={scales!r}: expected a sequence of numbers") from None
    for s in scales:
        if not math.isfinite(s) or not 0.0 < s < 1.0:
            raise ValueError(f"train_scales: scale {s} is not a finite number in (0, 1): a copy is smaller than its image (1 would duplicate it)")
    if isinstance(short_side, float) and not short_side.is_integer():
        raise ValueError(f"train_short_side={short_side}: expected a whole number of pixels")
    short_side = int(short_side)
    if short_side < 0:
        raise ValueError(f"train_short_side={short_side} is negative: expected 0 (no such copy) or the shorter side of the copy")
    return scales, short_side


def train_copies():
    """The multi-scale copies of the whole-image data sources as (scales, short_side): `train_scales` -- a string as RESR_TRAIN_SCALES gives
    it ("0.75,0.5,1/3") or a sequence of numbers -- and `train_short_side`, checked by check_train_copies."""
    scales = train_scales
    if isinstance(scales, str):
        parsed = []
        for item in (part.strip() for part in scales.split(",")):
            if not item:
                continue
            try:
                top, _, bottom = item.partition("/")
                parsed.append(float(top) / float(bottom) if bottom else float(top))
            except (ValueError, ZeroDivisionError):
                raise ValueError(f"train_scales={scales!r} (RESR_TRAIN_SCALES): {item!r} is neither a number nor a/b") from None
        scales = parsed
    return check_train_copies(scales, train_short_side)


if data_source in IMAGE_DATA_SOURCES and mode in ("train_realesrnet", "train_realesrgan"):
    train_window()
    train_copies()


def pair_pool() -> int:
    """The size of the training pair pool, 0 = off: `pair_pool_size`, which must be a multiple of batch_size (the pool fills and
    exchanges in whole batches)."""
    if pair_pool_size < 0 or (pair_pool_size and pair_pool_size % batch_size):
        raise ValueError(f"config.pair_pool_size={pair_pool_size} (RESR_PAIR_POOL) is not a multiple of batch_size={batch_size}: the training "
                         "pair pool fills and exchanges in whole batches")
    return pair_pool_size


if mode in ("train_realesrnet", "train_realesrgan"):
    pair_pool()


def train_precision() -> str:
    """The training modules' precision: exact16 in output-parity mode, `precision` otherwise."""
    return "exact16" if output_parity else precision


def generator_options() -> dict:
    """Keyword arguments of the training Generator (train_realesrnet.py, train_realesrgan.py)."""
    from . import _lib
    opts = {"precision": train_precision()}
    if output_parity:
        opts["x2_plan"] = _lib.X2_PLAN_OUTPUT_PARITY
    return opts


def build_generator(training: bool):
    """The generator of `g_arch`, not yet on a device: the training module of the train scripts' build_model() (training=True) or
    the fp32 call site of test.py (training=False: `inference_precision`)."""
    if g_arch == "compact":
        from .compact import SRVGGNetCompact
        return SRVGGNetCompact(num_conv=compact_num_conv, upscale=upscale_factor, act_type=compact_act_type,
                               precision=train_precision() if training else inference_precision, trainable=training)
    if g_arch != "rrdb":
        raise ValueError(f"config.g_arch={g_arch!r}: expected 'rrdb' or 'compact'")
    from .model import Generator
    if training:
        return Generator(in_channels, out_channels, upscale_factor, **generator_options())        # (output parity: above)
    return Generator(in_channels, out_channels, upscale_factor, precision=inference_precision)    # fp32 call site: test.py:79-80 (no autocast)


def build_niqe():
    """The NIQE module of `niqe_backend` (and `niqe_tail`) on `device`: NIQE(upscale_factor, niqe_model_path) of the train scripts and test.py."""
    from .image_quality_assessment import NIQE, NativeNIQE
    if niqe_backend not in ("torch", "native"):
        raise ValueError(f"config.niqe_backend={niqe_backend!r}: expected 'torch' or 'native'")
    if niqe_tail not in ("torch", "native"):
        raise ValueError(f"config.niqe_tail={niqe_tail!r}: expected 'torch' or 'native'")
    if niqe_backend == "native":
        return NativeNIQE(upscale_factor, niqe_model_path, tail=niqe_tail).to(device=device)
    if niqe_tail == "native":
        raise ValueError("config.niqe_tail='native' needs config.niqe_backend='native': the torch backend has no native tail")
    return NIQE(upscale_factor, niqe_model_path).to(device=device)


def build_full_ref():
    """None for `full_ref` = "off", else a module on `device` with forward(sr, hr) -> (psnr [B], ssim [B]), crop_border = upscale_factor:
    of the Y channel, or with `full_ref_channels` = "rgb" (psnr over the three channels, mean of the channels' ssim)."""
    from .image_quality_assessment import NativeFullRef, NativeFullRefChannels, TorchFullRef, TorchFullRefChannels
    if full_ref not in ("off", "torch", "native"):
        raise ValueError(f"config.full_ref={full_ref!r}: expected 'off', 'torch' or 'native'")
    if full_ref_channels not in ("y", "rgb"):
        raise ValueError(f"config.full_ref_channels={full_ref_channels!r}: expected 'y' or 'rgb'")
    if full_ref == "off":
        return None
    modules = {"y": (TorchFullRef, NativeFullRef), "rgb": (TorchFullRefChannels, NativeFullRefChannels)}[full_ref_channels]
    return modules[full_ref == "native"](upscale_factor).to(device=device)


def backward_options() -> dict:
    """Keyword arguments of the training Discriminator and ContentLoss."""
    opts = {"precision": train_precision()}
    if output_parity:
        opts["f16_backward"] = True
    return opts
