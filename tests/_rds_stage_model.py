"""NumPy float64 model of the RDS chain's stages that use only multiply and add (csrc/rds_bank.hip), in the kernels' order of
operations: one product and one sum per step.  NumPy does not fuse a product into a sum and the library is built with
-ffp-contract=off, so each stage equals the kernel's output bit for bit when it is fed what the kernel was fed.  Every stage
therefore takes the DEVICE's tap of the stage before it as input, and the model carries the histories from the previous
blocks' inputs and taps (the device carries them as raw samples in front of each row):

  channel      acc = h[j] * x[k-j] + acc, j = taps-1 .. 0, on the float32 input widened to float64     rdsb_fir_kernel<0>
  carrier      the same FIR on the square of the channel tap                                           rdsb_fir_kernel<1>
  mi, mq       pll_i[i] * channel[i - delay] * 2, pll_q likewise                                       rdsb_mix_kernel
  resampled_i  acc = acc + h[ph + jU] * mi[b - j], j = 0 .. 100, then * U; b = kD // U, ph = kD % U     rdsb_resample_kernel
  rrc_i        the FIR of the resampled_i tap
  rrc_q        the resampler on mq, then the FIR (the device has no tap in between)

The PLL's recurrence calls atan2 / sincos and is not modelled: its rows are inputs here."""
import numpy as np


def fir(h, hist, x, square=False):
    """y[k] = sum_j h[j] x[k-j] in the device's order; hist: the len(h)-1 samples before x."""
    xx = np.concatenate([hist, x])
    if square:
        xx = xx * xx
    H, n = len(h) - 1, len(x)
    acc = np.zeros(n)
    for j in range(H, -1, -1):
        acc = h[j] * xx[H - j:H - j + n] + acc
    return acc


def resample(h, hist, x, U, D):
    """convolveBlockResampleFIR in stream form, gain U, in the device's order; hist: the (len(h)-1)//U samples before x."""
    xx = np.concatenate([hist, x])
    m = np.arange(len(x) * U // D, dtype=np.int64) * D
    ph, b = m % U, len(hist) + m // U
    assert len(h) % U == 0                              # the same number of steps for every phase
    acc = np.zeros(len(m))
    for j in range(len(h) // U):
        acc = acc + h[ph + j * U] * xx[b - j]
    return acc * float(U)


class StageModel:
    """h_ch, h_car, h_rs, h_rrc: the four filters the chain under test uses (its own host designs)."""

    def __init__(self, U, D, h_ch, h_car, h_rs, h_rrc):
        self.U, self.D = U, D
        self.h_ch, self.h_car, self.h_rs, self.h_rrc = (np.asarray(h, np.float64) for h in (h_ch, h_car, h_rs, h_rrc))
        self.delay = (len(self.h_ch) - 1) // 2
        self.x = np.zeros(len(self.h_ch) - 1)
        self.ch = np.zeros(len(self.h_car) - 1)
        self.mi = np.zeros((len(self.h_rs) - 1) // U)
        self.mq = self.mi.copy()
        self.ri = np.zeros(len(self.h_rrc) - 1)
        self.rq = self.ri.copy()

    @staticmethod
    def _carry(hist, x):
        return np.concatenate([hist, x])[len(x):]

    def step(self, x, dev):
        """x: the block's float32 input; dev: the taps of this block (channel, pll_i, pll_q, resampled_i) of the chain under
        test.  -> what channel, carrier, resampled_i, rrc_i and rrc_q must then be."""
        x = np.asarray(x, np.float32).astype(np.float64)
        n, ch = len(x), np.asarray(dev["channel"], np.float64)
        exp = {"channel": fir(self.h_ch, self.x, x), "carrier": fir(self.h_car, self.ch, ch, square=True)}
        ap = np.concatenate([self.ch, ch])[len(self.ch) - self.delay:][:n]
        mi, mq = dev["pll_i"][:n] * ap * 2, dev["pll_q"][:n] * ap * 2
        exp["resampled_i"] = resample(self.h_rs, self.mi, mi, self.U, self.D)
        rq = resample(self.h_rs, self.mq, mq, self.U, self.D)
        ri = np.asarray(dev["resampled_i"], np.float64)
        exp["rrc_i"] = fir(self.h_rrc, self.ri, ri)
        exp["rrc_q"] = fir(self.h_rrc, self.rq, rq)
        self.x, self.ch = self._carry(self.x, x), self._carry(self.ch, ch)
        self.mi, self.mq = self._carry(self.mi, mi), self._carry(self.mq, mq)
        self.ri, self.rq = self._carry(self.ri, ri), self._carry(self.rq, rq)
        return exp


def stage_model(fmrx, p):
    """The model with the filters the handle uploads (the host designs of the public ABI)."""
    return StageModel(p.upsamp, p.decim, fmrx.rdsBandPass(p.taps, p.if_Fs, 54e3, 60e3), fmrx.rdsBandPass(p.taps, p.if_Fs, 113.5e3, 114.5e3),
                      fmrx.rdsImpResponse(101 * p.upsamp, float(p.if_Fs) * p.upsamp, 3e3),
                      fmrx.impulseResponseRootRaisedCosine(2375.0 * p.sps, p.rrc_taps))
