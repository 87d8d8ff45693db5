"""Golden vectors of the SparseCtrl image-condition variant (configs/inference/sparsectrl/image_condition.yaml) from the REFERENCE's own
``SparseControlNetModel`` on the tiny U-Net geometry -> tests/golden/sparsectrl_image_tiny.npz.

Runs only where the reference sources are (it imports them through oracle.gen_golden's scaffolding); the tests read the stored
inputs and outputs only.  Weights: ``random_state_dict(..., zero_init_heads=False)``, so the embedding's ``conv_out`` is NOT zero and
the embedding reaches every residual.

Usage:  python tools/gen_golden_sparsectrl_image.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

IMAGE_CONDITION_KWARGS = dict(
    set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=False, conditioning_channels=3,
    use_motion_module=True, motion_module_resolutions=[1, 2, 4, 8], motion_module_mid_block=False, motion_module_type="Vanilla",
    motion_module_kwargs=dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self"],
                              temporal_position_encoding=True, temporal_position_encoding_max_len=32, temporal_attention_dim_div=1))
COND_FRAMES = (0, 5)


@torch.no_grad()
def main():
    from oracle.gen_golden import build_reference_unet, reference_classes
    from tiny_configs import tiny_unet_config
    from neurons_amd import _lib
    from neurons_amd.synth import randn
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.unet3d import random_state_dict

    ucfg = tiny_unet_config()
    ccfg = controlnet_config_from_unet(ucfg, IMAGE_CONDITION_KWARGS)
    usd = random_state_dict(ucfg, _lib.NR_KIND_UNET3D, seed=11)
    csd = random_state_dict(ccfg, _lib.NR_KIND_SPARSECTRL, seed=13, zero_init_heads=False)
    _, Ctrl, _, _, _ = reference_classes()
    mm = dict(ccfg.motion_module_kwargs)
    mm["attention_block_types"] = list(mm["attention_block_types"])
    ctrl = Ctrl(in_channels=ccfg.in_channels, conditioning_channels=ccfg.conditioning_channels,
                down_block_types=tuple(ccfg.down_block_types), block_out_channels=tuple(ccfg.block_out_channels),
                layers_per_block=ccfg.layers_per_block, norm_num_groups=ccfg.norm_num_groups, norm_eps=ccfg.norm_eps,
                cross_attention_dim=ccfg.cross_attention_dim, attention_head_dim=ccfg.attention_head_dim,
                use_motion_module=True, motion_module_resolutions=(1, 2, 4, 8), motion_module_mid_block=False,
                motion_module_type="Vanilla", motion_module_kwargs=mm, concate_conditioning_mask=True,
                conditioning_embedding_out_channels=tuple(ccfg.conditioning_embedding_out_channels),
                use_simplified_condition_embedding=False, set_noisy_sample_input_to_zero=True)
    ref_keys = sorted(k for k in ctrl.state_dict().keys() if not k.endswith("pos_encoder.pe"))
    assert ref_keys == sorted(csd.keys()), "schema differs from the reference's state_dict keys"
    missing, unexpected = ctrl.load_state_dict(csd, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("pos_encoder.pe") for k in missing), missing
    ctrl = ctrl.eval()
    unet = build_reference_unet(ucfg, usd)

    # one sample (no CFG pair): the full fp32 residuals of a CFG batch would not fit the 1 MiB a fixture may have
    B, F, H, W = 1, 8, 8, 8
    up = 8
    sample = randn("img.sample", (B, 4, F, H, W), 31)
    ctx = randn("img.ctx", (B, 77, ucfg.cross_attention_dim), 32)
    cond = torch.zeros(B, 3, F, H * up, W * up)
    mask = torch.zeros(B, 1, F, H * up, W * up)
    for i, f in enumerate(COND_FRAMES):
        cond[:, :, f] = randn(f"img.cond{i}", (B, 3, H * up, W * up), 33 + i).clamp(-2, 2) * 0.5
        mask[:, :, f] = 1
    t = 681

    emb = {}
    hook = ctrl.controlnet_cond_embedding.register_forward_hook(lambda m, i, o: emb.__setitem__("out", o))
    down, mid = ctrl(sample, t, encoder_hidden_states=ctx, controlnet_cond=cond, conditioning_mask=mask, conditioning_scale=1.0,
                     guess_mode=False, return_dict=False)
    hook.remove()
    eps_ctrl = unet(sample, t, encoder_hidden_states=ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
    out = dict(sample=sample.numpy(), ctx=ctx.numpy(), cond=cond.numpy(), mask=mask.numpy(), t=np.int64(t),
               cond_frames=np.array(COND_FRAMES, dtype=np.int64), embedding=emb["out"].numpy(), mid_res=mid.numpy(),
               eps_ctrl=eps_ctrl.numpy(), ctrl_seed=np.int64(13), unet_seed=np.int64(11), ref_keys=np.array(ref_keys),
               ref_shapes=np.array([",".join(str(d) for d in ctrl.state_dict()[k].shape) for k in ref_keys]))
    for i, d in enumerate(down):
        out[f"down_res_{i}"] = d.numpy()
    path = os.path.join(ROOT, "tests", "golden", "sparsectrl_image_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    main()
