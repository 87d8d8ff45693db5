"""SparseCtrl image-condition variant (configs/inference/sparsectrl/image_condition.yaml), host side: config checks, the C config,
the state-dict schema against the reference's key list, the zero-init rule, and the fp32 restatement the GPU tests use, pinned on
the reference fixture tests/golden/sparsectrl_image_tiny.npz (tools/gen_golden_sparsectrl_image.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sparsectrl_image_tiny.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from sparsectrl_image_ref import IMAGE_CONDITION_KWARGS, sparsectrl_image_forward, tiny_image_ctrl_config  # noqa: E402


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def test_image_condition_config_is_supported_and_excluded_options_still_raise():
    from neurons_amd import _lib
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.unet3d import UNet3DConfig, condition_upscale, make_c_config
    cfg = controlnet_config_from_unet(UNet3DConfig(), IMAGE_CONDITION_KWARGS)
    assert cfg.conditioning_embedding_out_channels == (16, 32, 96, 256) and cfg.conditioning_channels == 3
    assert condition_upscale(cfg) == 8
    c = make_c_config(cfg, _lib.NR_KIND_SPARSECTRL)
    assert c.cond_embedding_levels == 4 and list(c.cond_embedding_channels) == [16, 32, 96, 256] and c.conditioning_channels == 3
    # the latent variant keeps the simplified single conv: the new fields stay 0
    lat = controlnet_config_from_unet(UNet3DConfig(), dict(IMAGE_CONDITION_KWARGS, use_simplified_condition_embedding=True,
                                                            conditioning_channels=4))
    c = make_c_config(lat, _lib.NR_KIND_SPARSECTRL)
    assert c.cond_embedding_levels == 0 and list(c.cond_embedding_channels) == [0, 0, 0, 0] and condition_upscale(lat) == 1
    custom = controlnet_config_from_unet(UNet3DConfig(), dict(IMAGE_CONDITION_KWARGS, conditioning_embedding_out_channels=[16, 32, 64]))
    assert make_c_config(custom, _lib.NR_KIND_SPARSECTRL).cond_embedding_levels == 3 and condition_upscale(custom) == 4
    with pytest.raises(NotImplementedError):
        make_c_config(controlnet_config_from_unet(UNet3DConfig(), dict(IMAGE_CONDITION_KWARGS, concate_conditioning_mask=False)),
                      _lib.NR_KIND_SPARSECTRL)
    with pytest.raises(NotImplementedError):
        make_c_config(controlnet_config_from_unet(UNet3DConfig(), dict(IMAGE_CONDITION_KWARGS, use_simplified_condition_embedding=True,
                                                                        concate_conditioning_mask=False)), _lib.NR_KIND_SPARSECTRL)
    with pytest.raises(NotImplementedError):
        make_c_config(controlnet_config_from_unet(UNet3DConfig(), dict(IMAGE_CONDITION_KWARGS, conditioning_embedding_out_channels=(8, 32))),
                      _lib.NR_KIND_SPARSECTRL)
    for bad in ("global_pool_conditions", "controlnet_conditioning_channel_order"):
        with pytest.raises(TypeError):
            controlnet_config_from_unet(UNet3DConfig(), dict(IMAGE_CONDITION_KWARGS, **{bad: False}))


def test_schema_embedding_keys_match_the_reference_key_list():
    from neurons_amd import _lib
    from neurons_amd.unet3d import state_dict_schema
    g = np.load(GOLD)
    ref = {str(k): tuple(int(d) for d in str(s).split(",")) for k, s in zip(g["ref_keys"], g["ref_shapes"])}
    schema = state_dict_schema(tiny_image_ctrl_config(), _lib.NR_KIND_SPARSECTRL)
    assert schema == ref
    emb = {k: v for k, v in schema.items() if k.startswith("controlnet_cond_embedding.")}
    assert len(emb) == 16 and "controlnet_cond_embedding.weight" not in schema
    assert emb["controlnet_cond_embedding.conv_in.weight"] == (16, 4, 3, 3)
    assert emb["controlnet_cond_embedding.blocks.5.weight"] == (256, 96, 3, 3)
    assert emb["controlnet_cond_embedding.conv_out.weight"] == (64, 256, 3, 3)


def test_random_state_dict_zero_inits_only_the_embedding_conv_out():
    from neurons_amd import _lib
    from neurons_amd.unet3d import random_state_dict
    sd = random_state_dict(tiny_image_ctrl_config(), _lib.NR_KIND_SPARSECTRL, seed=3, zero_init_heads=True)
    for k, v in sd.items():
        if k.startswith("controlnet_cond_embedding.conv_out."):
            assert not v.any(), k
        elif k.startswith("controlnet_cond_embedding."):
            assert v.abs().sum() > 0, k
    sd = random_state_dict(tiny_image_ctrl_config(), _lib.NR_KIND_SPARSECTRL, seed=3, zero_init_heads=False)
    assert all(v.abs().sum() > 0 for k, v in sd.items() if k.startswith("controlnet_cond_embedding."))


@torch.no_grad()
def test_fp32_restatement_matches_the_reference_fixture():
    from neurons_amd import _lib
    from neurons_amd.unet3d import random_state_dict
    g = np.load(GOLD)
    cfg = tiny_image_ctrl_config()
    sd = random_state_dict(cfg, _lib.NR_KIND_SPARSECTRL, seed=int(g["ctrl_seed"]), zero_init_heads=False)
    assert sd["controlnet_cond_embedding.conv_out.weight"].abs().sum() > 0
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    e, down, mid = sparsectrl_image_forward(sd, cfg, t("sample"), int(g["t"]), t("ctx"), t("cond"), t("mask"))
    assert _rel(e, g["embedding"]) < 1e-5
    assert len(down) == 12
    for i, d in enumerate(down):
        assert _rel(d, g[f"down_res_{i}"]) < 1e-5, i
    assert _rel(mid, g["mid_res"]) < 1e-5
    # the embedding reaches the residuals: without it (zero condition and mask) they move
    e0, down0, _ = sparsectrl_image_forward(sd, cfg, t("sample"), int(g["t"]), t("ctx"), t("cond") * 0, t("mask") * 0)
    assert _rel(down0[0], g["down_res_0"]) > 1e-2
