"""Host mirror of bitrate_selection/utils/qoe.py:10-47 for ONE session: `QoEModel.calculate_qoe` restated in numpy float32 with the
reference's sequential sums in tile order (Python `sum` over a float32 array).  It is what a caller of the single-session `Simulator`
pairs it with; the batched path (`BatchedSimulator`, `MANSYVecEnv`) gets the same four numbers from the kernel, bit for bit."""
import numpy as np

# to ensure that the all QoE metrics are in the same/similar scales (qoe.py:5-7)
SCALE_QUALITY = 1
SCALE_VARIANCE = 1
SCALE_REBUFFER = 1

_F = np.float32


def _seq_sum(x):
    s = _F(0.0)
    for v in x:
        s = _F(s + v)
    return s


class QoEModel:
    def __init__(self, config, weight1, weight2, weight3):
        self.config = config
        self.reset_with_new_weights(weight1, weight2, weight3)

    def calculate_qoe(self, actual_viewport, tile_quality, rebuffer_time):
        """-> (qoe, qoe1, qoe2, qoe3): np.float32 except qoe2, which is `rebuffer_time` as passed (qoe.py:31,34)."""
        av = np.asarray(actual_viewport, dtype=_F).reshape(-1)
        tq = np.asarray(tile_quality, dtype=_F).reshape(-1)
        max_rate = _F(self.config.video_rates[-1])
        s_v = _seq_sum(av)
        with np.errstate(divide='ignore', invalid='ignore'):       # an empty viewport is NaN in the reference too
            viewport_quality = _F(_seq_sum(av * tq) / s_v)
            intra = _F(_F(_seq_sum(av * np.abs(tq - viewport_quality)) / s_v) / max_rate)
        viewport_quality = _F(viewport_quality / max_rate)
        inter = _F(abs(_F(viewport_quality - self.prev_viewport_quality))) if self.prev_viewport_quality is not None else _F(0.0)
        self.prev_viewport_quality = viewport_quality
        self.prev_rebuffer_time = rebuffer_time
        self.qoe1 = _F(viewport_quality * _F(SCALE_QUALITY))
        self.qoe2 = rebuffer_time * SCALE_REBUFFER
        self.qoe3 = _F(_F(intra + inter) * _F(SCALE_VARIANCE))
        qoe = _F(_F(_F(self.weight1 * self.qoe1) - _F(self.weight2 * _F(self.qoe2))) - _F(self.weight3 * self.qoe3))
        return qoe, self.qoe1, self.qoe2, self.qoe3

    def reset(self):
        self.qoe1 = 0.0
        self.qoe2 = 0.0
        self.qoe3 = 0.0
        self.prev_viewport_quality = None
        self.prev_rebuffer_time = 0.0

    def reset_with_new_weights(self, weight1, weight2, weight3):
        self.weight1, self.weight2, self.weight3 = _F(weight1), _F(weight2), _F(weight3)
        self.reset()
