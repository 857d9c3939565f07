"""Multi-ControlNet and guidance windows, restated on the CPU -- a helper, not a test file.

* ``control_residuals_cpu``: what ``ed_control_residuals`` computes for one level, as the torch-CPU fp32 op sequence
  (``acc = acc + w * r``: one rounded product, one rounded sum, per net in order; one cast at the end).  A zero weight leaves its
  term out, so a non-finite value in a closed net does not reach the output.
* ``control_keep``: diffusers 0.21.4's ``controlnet_keep`` table.
* ``MultiControlNetSpec``: diffusers' ``MultiControlNetModel`` with the guidance window folded in, as a callable with the signature
  of ONE ControlNet: the condition rows of the N nets arrive stacked along the channels, ``conditioning_scale`` is the list of N
  scales, and the step index is looked up from ``t`` in the list of executed timesteps.  ``oracle/elastic_oracle.py`` is
  channel-agnostic in the condition image, passes the scale through and hands ``t`` to its ControlNet: the unchanged oracle with
  this wrapper is the end-to-end specification.
"""
import torch


def control_residuals_cpu(skip, residuals, w, out_dtype=None):
    """skip: tensor [B, ...] or None; residuals: N tensors of that shape; w: [B, N] -> out in ``out_dtype`` (default: the skip's
    type, the residuals' without a skip)."""
    r0 = residuals[0]
    B = r0.shape[0]
    acc = torch.zeros(r0.shape, dtype=torch.float32) if skip is None else skip.detach().cpu().to(torch.float32).clone()
    w = w.detach().cpu().to(torch.float32)
    for n, r in enumerate(residuals):
        r = r.detach().cpu()
        for b in range(B):
            if float(w[b, n]) != 0.0:
                acc[b] = acc[b] + w[b, n] * r[b].to(torch.float32)
    return acc.to(out_dtype or (r0.dtype if skip is None else skip.dtype))


def control_keep(n_steps, start, end):
    """keep[i][n] = 1.0 - float(i / T < start[n] or (i + 1) / T > end[n]) for T = ``n_steps`` executed timesteps"""
    return [[1.0 - float(i / n_steps < s or (i + 1) / n_steps > e) for s, e in zip(start, end)] for i in range(n_steps)]


class MultiControlNetSpec(torch.nn.Module):
    def __init__(self, nets, timesteps, start=None, end=None):
        """``nets``: N ControlNet callables; ``timesteps``: the EXECUTED timesteps in order (after ``strength``)"""
        super().__init__()
        self.nets = torch.nn.ModuleList(nets) if all(isinstance(n, torch.nn.Module) for n in nets) else list(nets)
        N = len(nets)
        self.timesteps = [int(t) for t in timesteps]
        self.keep = control_keep(len(self.timesteps), start or [0.0] * N, end or [1.0] * N)
        self.calls = [0] * N

    def forward(self, x, t, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0, **kw):
        N = len(self.nets)
        assert controlnet_cond.shape[1] == 3 * N
        scales = list(conditioning_scale) if isinstance(conditioning_scale, (list, tuple)) else [conditioning_scale] * N
        keep = self.keep[self.timesteps.index(int(t))]
        down_sum = mid_sum = None
        for n, net in enumerate(self.nets):
            # diffusers: cond_scale = scale * keep; MultiControlNetModel.forward sums the nets' scaled lists
            scale = scales[n] * keep[n]
            down, mid = net(x, t, encoder_hidden_states=encoder_hidden_states, controlnet_cond=controlnet_cond[:, 3 * n:3 * n + 3],
                            conditioning_scale=scale, **kw)
            self.calls[n] += 1
            if down_sum is None:
                down_sum, mid_sum = list(down), mid
            else:
                down_sum = [a + b for a, b in zip(down_sum, down)]
                mid_sum = mid_sum + mid
        return down_sum, mid_sum
