"""What the method benchmarks (bench_sar.py, bench_memo.py, bench_cotta.py) share: the bench U-Net, `lanes` plugins of one
method adapting the same seeded volumes, and the build / warm-up / timed rounds / release of one method."""
import gc
import time

import torch

MODEL = dict(name="unet", in_channels=4, num_classes=3, spatial_dims=3, channels=[32, 64, 128, 256, 512],
             strides=[2, 2, 2, 2], num_res_units=2, norm="INSTANCE", act="RELU", dropout=0.0)
AXES = {1: [], 2: ["w"], 4: ["h", "w"], 8: ["d", "h", "w"]}          # mirror axes by number of views


class Method:
    """`lanes` plugins (own model replica, stream and graph each) adapting `group` volumes per launch sequence.
    `section`: (key, values) written over that section of the method's config (``method.sar``, ``method.memo``, ...);
    `plugin`: a registered plugin name to run that config with instead of its own ``method.name``; `overrides`: further keys
    of ``method`` itself (``params``, ...)."""

    def __init__(self, method, lanes, group, streams, device, steps, section=None, plugin=None, overrides=None):
        from multimodal_tta_amd.config import compose
        from multimodal_tta_amd.models import UNet
        from multimodal_tta_amd.registry import get_plugin

        self.lanes, self.group = lanes, group
        cfg = compose(overrides=["task=brats", "model=unet", f"method={method}"])
        cfg["model"] = dict(MODEL)
        cfg["method"].update(steps=steps, precision="bf16", group=group, lanes=lanes)
        if section is not None:
            cfg["method"][section[0]].update(section[1])
        if plugin is not None:
            cfg["method"]["name"] = plugin
        if overrides:
            cfg["method"].update(overrides)
        self.streams = streams[:lanes]
        self.plugs = []
        self.result = None          # lane 0's result of the last round
        for lane in range(lanes):
            torch.manual_seed(42)
            p = get_plugin(str(cfg["method"]["name"]))(cfg)
            p.lane = lane
            self.plugs.append(p.setup(UNet(dict(MODEL)), device))

    def round(self, xs):
        for lane in range(self.lanes):
            lo = lane * self.group
            with torch.cuda.stream(self.streams[lane]):
                r = self.plugs[lane].adapt_volume(xs[lo:lo + self.group])
            if lane == 0:
                self.result = r
        return self.lanes * self.group


def measure(make, xs, volumes, device):
    """Build a method, warm it up, time at least `volumes` volumes, release it: (volumes/s, peak memory in GB, volumes)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(device)
    m = make()
    m.round(xs)                                         # warm-up: capture
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while n < volumes:
        n += m.round(xs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated(device) / 2 ** 30
    del m
    gc.collect()
    torch.cuda.empty_cache()
    return round(n / dt, 2), round(peak, 2), n
