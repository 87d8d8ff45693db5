"""Schema file for tests/sanitize/plan_dump.cpp (tools/plan_equal.sh): the networks of the sanitizer dry-run (tests/test_sanitize_host.py) plus the
SparseCtrl image-condition variant, the C = 1280 leaf modules and the tiny U-Net / SparseCtrl variants that reach the builder's remaining branches.  Needs no GPU.  usage: python tools/plan_schema.py <out-file>"""
import os
import sys
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neurons_amd import _lib  # noqa: E402
from neurons_amd.unet3d import _motion_keys, _transformer_keys, make_c_config, state_dict_schema  # noqa: E402
from sparsectrl_image_ref import tiny_image_ctrl_config  # noqa: E402
from test_sanitize_host import _cfg_words, _write_schema  # noqa: E402
from tiny_configs import tiny_ctrl_config, tiny_unet_config  # noqa: E402


def leaf1280(name, kind, keys):      # as the dry-run's leaf networks, at C = 1280
    c = _lib.NrNetConfig()
    c.kind = kind
    c.in_channels = c.out_channels = c.block_out_channels[0] = 1280
    c.num_levels = 1
    c.num_heads, c.cross_attention_dim, c.norm_num_groups, c.norm_eps = 8, 768, 32, 1e-5
    c.use_motion_module, c.motion_num_heads, c.motion_num_attention_blocks, c.motion_pe_max_len = 1, 8, 2, 24
    return name, c, keys


def net(name, cfg, kind):
    return name, make_c_config(cfg, kind), state_dict_schema(cfg, kind)


_write_schema(sys.argv[1])
with open(sys.argv[1], "a") as f:
    # the variants no other config reaches: the noisy sample not zeroed (both SparseCtrl stems), a motion module in the mid block, and more
    # residuals (16 skips + mid) than one multi-add launch takes
    for name, cconf, schema in (net("tiny_ctrl_image", tiny_image_ctrl_config(), _lib.NR_KIND_SPARSECTRL),
                                leaf1280("leaf_transformer1280", _lib.NR_KIND_LEAF_TRANSFORMER3D, _transformer_keys("m", 1280, 768)),
                                leaf1280("leaf_temporal1280", _lib.NR_KIND_LEAF_TEMPORAL, _motion_keys("m", 1280, 2)),
                                net("tiny_ctrl_noisy", replace(tiny_ctrl_config(), set_noisy_sample_input_to_zero=False), _lib.NR_KIND_SPARSECTRL),
                                net("tiny_ctrl_image_noisy", tiny_image_ctrl_config(set_noisy_sample_input_to_zero=False), _lib.NR_KIND_SPARSECTRL),
                                net("tiny_unet_midmotion", replace(tiny_unet_config(), motion_module_mid_block=True), _lib.NR_KIND_UNET3D),
                                net("tiny_unet_lpb3", replace(tiny_unet_config(), layers_per_block=3), _lib.NR_KIND_UNET3D)):
        f.write("N " + name + " " + " ".join(str(w) for w in _cfg_words(cconf)) + "\n")
        for k, shape in schema.items():
            f.write(f"T {k} {len(shape)} " + " ".join(str(int(d)) for d in shape) + "\n")
