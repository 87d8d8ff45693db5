"""Schema file for tests/sanitize/plan_dump.cpp (tools/plan_equal.sh): the networks of the sanitizer dry-run (tests/test_sanitize_host.py) plus the
SparseCtrl image-condition variant and the C = 1280 leaf modules.  Needs no GPU.   usage: python tools/plan_schema.py <out-file>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neurons_amd import _lib  # noqa: E402
from neurons_amd.unet3d import _motion_keys, _transformer_keys, make_c_config, state_dict_schema  # noqa: E402
from sparsectrl_image_ref import tiny_image_ctrl_config  # noqa: E402
from test_sanitize_host import _cfg_words, _write_schema  # noqa: E402


def leaf1280(name, kind, keys):      # as the dry-run's leaf networks, at C = 1280
    c = _lib.NrNetConfig()
    c.kind = kind
    c.in_channels = c.out_channels = c.block_out_channels[0] = 1280
    c.num_levels = 1
    c.num_heads, c.cross_attention_dim, c.norm_num_groups, c.norm_eps = 8, 768, 32, 1e-5
    c.use_motion_module, c.motion_num_heads, c.motion_num_attention_blocks, c.motion_pe_max_len = 1, 8, 2, 24
    return name, c, keys


icfg = tiny_image_ctrl_config()
_write_schema(sys.argv[1])
with open(sys.argv[1], "a") as f:
    for name, cconf, schema in (("tiny_ctrl_image", make_c_config(icfg, _lib.NR_KIND_SPARSECTRL), state_dict_schema(icfg, _lib.NR_KIND_SPARSECTRL)),
                                leaf1280("leaf_transformer1280", _lib.NR_KIND_LEAF_TRANSFORMER3D, _transformer_keys("m", 1280, 768)),
                                leaf1280("leaf_temporal1280", _lib.NR_KIND_LEAF_TEMPORAL, _motion_keys("m", 1280, 2))):
        f.write("N " + name + " " + " ".join(str(w) for w in _cfg_words(cconf)) + "\n")
        for k, shape in schema.items():
            f.write(f"T {k} {len(shape)} " + " ".join(str(int(d)) for d in shape) + "\n")
