"""fp32 restatement of the SparseCtrl image-condition variant (configs/inference/sparsectrl/image_condition.yaml), built from the pinned
oracle's blocks plus SparseControlNetConditioningEmbedding (animatediff/models/sparse_controlnet.py:49-82,513-521).  Pinned against the
reference fixture tests/golden/sparsectrl_image_tiny.npz on CPU (test_sparsectrl_image_host.py); the full-width GPU tests compare the
engine with it.  Plain configuration and torch: no reference import."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import animatediff_oracle as O  # noqa: E402

IMAGE_CONDITION_KWARGS = dict(
    set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=False, conditioning_channels=3,
    use_motion_module=True, motion_module_resolutions=[1, 2, 4, 8], motion_module_mid_block=False, motion_module_type="Vanilla",
    motion_module_kwargs=dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self"],
                              temporal_position_encoding=True, temporal_position_encoding_max_len=32, temporal_attention_dim_div=1))


def image_ctrl_config(unet_config, **overrides):
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    kw = dict(IMAGE_CONDITION_KWARGS)
    kw.update(overrides)
    return controlnet_config_from_unet(unet_config, kw)


def tiny_image_ctrl_config(**overrides):
    from tiny_configs import tiny_unet_config
    return image_ctrl_config(tiny_unet_config(), **overrides)


def cond_embedding(sd, levels, cond, mask):
    """SparseControlNetConditioningEmbedding.forward on cat([cond, mask]) (b, c + 1, f, 8h, 8w) -> (b, C0, f, h, w)."""
    p = "controlnet_cond_embedding"
    x = F.silu(O.inflated_conv3d(torch.cat([cond, mask], dim=1), sd[f"{p}.conv_in.weight"], sd[f"{p}.conv_in.bias"]))
    for i in range(2 * (levels - 1)):
        x = F.silu(O.inflated_conv3d(x, sd[f"{p}.blocks.{i}.weight"], sd[f"{p}.blocks.{i}.bias"], stride=1 + i % 2))
    return O.inflated_conv3d(x, sd[f"{p}.conv_out.weight"], sd[f"{p}.conv_out.bias"])


def sparsectrl_image_forward(sd, cfg, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_mask, conditioning_scale=1.0):
    """SparseControlNetModel.forward (sparse_controlnet.py:467-581) with the image-condition embedding.  Returns (embedding, down, mid)."""
    ocfg = O.OracleConfig.from_native(cfg)
    if cfg.set_noisy_sample_input_to_zero:
        sample = torch.zeros_like(sample)
    ctx = encoder_hidden_states.repeat(sample.shape[0] // encoder_hidden_states.shape[0], 1, 1)
    emb = O._time_embedding(sd, ocfg, timestep, sample.shape[0], sample.device)
    x = O.inflated_conv3d(sample, sd["conv_in.weight"], sd["conv_in.bias"])
    e = cond_embedding(sd, len(cfg.conditioning_embedding_out_channels), controlnet_cond, conditioning_mask)
    reps = x.shape[0] // e.shape[0]
    x = x + (e if reps == 1 else e.repeat(reps, 1, 1, 1, 1))
    x, skips = O._down_blocks(sd, ocfg, x, emb, ctx)
    x = O._mid_block(sd, ocfg, x, emb, ctx)
    down = [O.inflated_conv3d(s, sd[f"controlnet_down_blocks.{i}.weight"], sd[f"controlnet_down_blocks.{i}.bias"], padding=0)
            * conditioning_scale for i, s in enumerate(skips)]
    mid = O.inflated_conv3d(x, sd["controlnet_mid_block.weight"], sd["controlnet_mid_block.bias"], padding=0) * conditioning_scale
    return e, down, mid
