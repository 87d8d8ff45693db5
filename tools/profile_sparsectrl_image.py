"""One SparseCtrl evaluation at config-2 shapes (SD-1.5 widths, one 16-frame clip at a 32 x 32 latent, CFG batch 2, condition on frame 0):
the image-condition variant (RGB keyframe at 256 x 256 through SparseControlNetConditioningEmbedding) against the latent-condition
variant (4-channel latent keyframe, the simplified single conv).  Synthetic weights (neurons_amd.synth.gpu_random_state_dict).

  python tools/profile_sparsectrl_image.py --time       evaluation time of both variants (hipGraph replay, device events, alternated)
  rocprofv3 --kernel-trace --stats -d OUT -o sc -- python tools/profile_sparsectrl_image.py --trace
                                                        eager launches of the image variant: one warm-up + one traced evaluation
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(variant, dev):
    from neurons_amd import _lib, NativeSparseCtrl
    from neurons_amd.sparsectrl import controlnet_config_from_unet
    from neurons_amd.synth import gpu_random_state_dict
    from neurons_amd.unet3d import UNet3DConfig, state_dict_schema
    kw = dict(set_noisy_sample_input_to_zero=True, motion_module_kwargs=dict(attention_block_types=["Temporal_Self"],
                                                                             temporal_position_encoding_max_len=32))
    if variant == "image":
        kw.update(use_simplified_condition_embedding=False, conditioning_channels=3)
    else:
        kw.update(use_simplified_condition_embedding=True, conditioning_channels=4)
    cfg = controlnet_config_from_unet(UNet3DConfig(), kw)
    sd = gpu_random_state_dict(state_dict_schema(cfg, _lib.NR_KIND_SPARSECTRL), 2, dev)
    net = NativeSparseCtrl(cfg).to(dev)
    net.load_state_dict({k: v.cpu() for k, v in sd.items()})
    F, L = 16, 32
    up = 8 if variant == "image" else 1
    g = torch.Generator(device=dev).manual_seed(0)
    cond = torch.zeros(1, cfg.conditioning_channels, F, L * up, L * up, device=dev)
    mask = torch.zeros(1, 1, F, L * up, L * up, device=dev)
    cond[:, :, 0] = torch.randn(1, cfg.conditioning_channels, L * up, L * up, generator=g, device=dev)
    mask[:, :, 0] = 1
    inp = dict(sample=torch.zeros(2, 4, F, L, L, device=dev), ctx=torch.randn(2, 77, 768, generator=g, device=dev), cond=cond, mask=mask)
    return net, inp


def evaluate(net, inp, t=501):
    return net(inp["sample"], t, encoder_hidden_states=inp["ctx"], controlnet_cond=inp["cond"], conditioning_mask=inp["mask"],
               return_dict=False, zero_copy=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.trace:
        net, inp = build("image", dev)
        net.enable_graph(False)
        evaluate(net, inp)
        torch.cuda.synchronize()
        evaluate(net, inp)
        torch.cuda.synchronize()
        for d in net.op_descriptions():
            if "condembed" in d:
                print(d)
        return
    nets = {v: build(v, dev) for v in ("latent", "image")}
    for net, inp in nets.values():
        for _ in range(5):
            evaluate(net, inp)
    torch.cuda.synchronize()
    times = {v: [] for v in nets}
    for rnd in range(4):                 # alternate the two variants
        for v, (net, inp) in nets.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                evaluate(net, inp)
            b.record()
            torch.cuda.synchronize()
            times[v].append(a.elapsed_time(b) / args.iters)
    for v, ts in times.items():
        print(f"{v}-condition SparseCtrl evaluation (2 x 16 f x 32^2, condition on frame 0): ms per evaluation "
              f"{' '.join(f'{t:.3f}' for t in ts)}  (min {min(ts):.3f})")
    print(f"image - latent: {min(times['image']) - min(times['latent']):+.3f} ms per evaluation (min vs min)")


if __name__ == "__main__":
    main()
