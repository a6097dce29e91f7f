"""What the three denoisers share on the MI355X: one iteration driver and the context's two ping-pong buffers.

The plain, the demodulated and the variance-guided denoise run back to back on ONE context and ONE stream of the caller's,
with no synchronisation between the calls of a film: all of them at 37 x 23, then at 130 x 70, then at 5 x 3, so the
ping-pong buffers grow and then serve a smaller film.  1, 2 and 5 iterations (at the default "denoise_lds_max_step" five
iterations take the LDS kernels for steps 1 and 2 and the global one for 4, 8 and 16), no iteration at all with a sample
table (the normalising kernel) and without one (the copy), and the plain one-iteration call in place.  Every output equals
the host instance bit for bit, and the guard words around every device buffer stay intact."""
import numpy as np
import pytest

from test_gpu_temporal import _between_guards, _payload
from test_variance import PIC, same_bits, vparams
from variance_ref import SIGMAS

pytestmark = pytest.mark.gpu
SIZES = ((37, 23), (130, 70), (5, 3))
SIGMA_COLOR = 0.7


def _calls(yk, p):
    """(name, params, samples, albedo, variance) of every out-of-place call on one film."""
    out = []
    for it in (1, 2, 5, 0):
        samples = p["samples"] if it in (0, 2) else None
        plain = yk.DenoiseParams(iterations=it, sigma_color=SIGMA_COLOR, sigma_normal=SIGMAS[1], sigma_plane=SIGMAS[2])
        out.append((f"plain-{it}", plain, samples, None, None))
        out.append((f"albedo-{it}", plain, samples, p["albedo"], None))
        out.append((f"variance-{it}", vparams(yk, it), samples, p["albedo"] if it != 2 else None, p["variance"]))
    out.append(("plain-0-copy", yk.DenoiseParams(iterations=0, sigma_color=SIGMA_COLOR, sigma_normal=SIGMAS[1], sigma_plane=SIGMAS[2]), None, None, None))
    return out


def test_three_denoisers_back_to_back_on_one_context_and_stream(ctx, yk):
    import torch

    s = torch.cuda.Stream()
    cs = s.cuda_stream
    for w, h in SIZES:
        p = PIC[(w, h)]
        n, res = w * h, (w, h)
        d_film, d_g = _between_guards(torch, 3 * n, 1, p["film"]), _between_guards(torch, 8 * n, 8, p["guides"])
        d_a, d_v = _between_guards(torch, 4 * n, 4, p["albedo"]), _between_guards(torch, n, 3, p["variance"])
        d_in_place = _between_guards(torch, 3 * n, 2, p["film"])
        calls = _calls(yk, p)
        outs = [_between_guards(torch, 3 * n, 1 + k % 4) for k in range(len(calls))]
        torch.cuda.synchronize()
        film, g, a, v = d_film.data_ptr() + 4, d_g.data_ptr() + 32, d_a.data_ptr() + 16, d_v.data_ptr() + 12
        for k, (name, par, samples, albedo, variance) in enumerate(calls):
            o = outs[k].data_ptr() + 4 * (1 + k % 4)
            if variance is not None:
                ctx.denoise_variance_device(film, g, v, res, par, 16, samples, o, stream=cs, albedo=None if albedo is None else a)
            else:
                ctx.denoise_device(film, g, res, par, 16, samples, o, stream=cs, albedo=None if albedo is None else a)
        one = calls[0][1]
        ctx.denoise_device(d_in_place.data_ptr() + 8, g, res, one, 16, None, d_in_place.data_ptr() + 8, stream=cs)
        s.synchronize()
        for k, (name, par, samples, albedo, variance) in enumerate(calls):
            want = yk.denoise(p["film"], p["guides"], par, tile_dim=16, samples=samples, albedo=albedo, variance=variance)
            got = _payload(outs[k], 1 + k % 4, 3 * n).view(np.float32)
            bad = got.view(np.uint32) != want.reshape(-1).view(np.uint32)
            assert not bad.any(), (name, res, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want.reshape(-1)[bad][:4])
        same_bits(_payload(d_in_place, 2, 3 * n).view(np.float32), yk.denoise(p["film"], p["guides"], one).reshape(-1))
        for t, lead, data in ((d_film, 1, p["film"]), (d_g, 8, p["guides"]), (d_a, 4, p["albedo"]), (d_v, 3, p["variance"])):
            assert np.array_equal(_payload(t, lead, data.nbytes // 4), np.ascontiguousarray(data).view(np.uint32).reshape(-1))  # only read
