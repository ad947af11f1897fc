"""The sample path between self-play and training, on the device (azmi_sample_loss / azmi_resample_plan / azmi_resample_gather,
csrc/samples_kernels.h): the reference's resample_by_surprise (game_runner.py:1148-1255) and the per-sample / per-iteration losses
behind it (NNWrapper.sample_loss, NNWrapper.losses, neural_net.py:644-676, 875-886), without the host round trip.

Every function takes numpy arrays (staged through the device) or CUDA tensors (in place, nothing leaves the device but the plan's
record) and answers in the kind it was given.  Argument errors are RuntimeErrors raised before any device call; inputs are
contiguous float32 (the losses: float64) and are never converted silently.  torch is imported inside the functions: importing
the package does not import it."""
import ctypes as C

import numpy as np

from ._capi import lib, ResampleRecordC

MAX_ROWS = 1 << 30
MAX_ENTRIES = 1 << 20


def _call(rc):
    if rc != 0:
        raise RuntimeError(lib.azmi_samples_last_error().decode("utf-8", "replace") or f"azmi error {rc}")


def _kind(what, named):
    """-> "numpy" | "torch" for the (name, array) pairs; all of one kind, tensors on one CUDA device"""
    kinds = set()
    for name, x in named:
        if isinstance(x, np.ndarray):
            kinds.add("numpy")
        elif hasattr(x, "is_cuda") and hasattr(x, "data_ptr"):
            kinds.add("torch")
        else:
            raise RuntimeError(f"{what}: {name} must be a numpy array or a CUDA tensor, got {type(x).__name__}")
    if len(kinds) > 1:
        raise RuntimeError(f"{what}: numpy arrays and tensors are mixed: " + ", ".join(f"{n} is a {type(x).__name__}" for n, x in named))
    kind = kinds.pop()
    if kind == "torch":
        for name, x in named:
            if not x.is_cuda:
                raise RuntimeError(f"{what}: {name} must be a CUDA tensor (numpy arrays take the staged path), it is on {x.device}")
        devs = {str(x.device) for _, x in named}
        if len(devs) > 1:
            raise RuntimeError(f"{what}: the arrays are on different devices: " + ", ".join(f"{n} on {x.device}" for n, x in named))
    return kind


def _check_dtype(what, name, x, want):
    """contiguous `want` ("float32", "float64", or a tuple of integer names), numpy or torch"""
    names = want if isinstance(want, tuple) else (want,)
    if isinstance(x, np.ndarray):
        ok, contiguous, have = x.dtype.name in names, x.flags.c_contiguous, x.dtype.name
    else:
        have = str(x.dtype).replace("torch.", "")
        ok, contiguous = have in names, bool(x.is_contiguous())
    if not ok or not contiguous:
        raise RuntimeError(f"{what}: {name} must be contiguous {' or '.join(names)}, got {'contiguous' if contiguous else 'non-contiguous'} {have}")


def _check_rows(what, n):
    if n > MAX_ROWS:
        raise RuntimeError(f"{what}: at most 2^30 rows, got {n}")


def _check_seed(what, seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise RuntimeError(f"{what}: seed must be an integer in [0, 2^64), got {seed!r}")
    return int(seed)


def _check_device(what, device):
    if isinstance(device, bool) or not isinstance(device, (int, np.integer)) or device < 0:
        raise RuntimeError(f"{what}: device must be a device index, got {device!r}")
    return int(device)


def _stage(x, device):
    import torch
    return torch.from_numpy(x).to(torch.device("cuda", device))


def _empty(shape, dtype, dev, stream):
    """A new tensor for work on `stream` (None: the current one).  torch's allocator hands a freed block back to the stream that was
    current at the allocation, so a tensor used on another stream is recorded there."""
    import torch
    t = torch.empty(shape, dtype=dtype, device=dev)
    if stream is not None and t.numel() and int(stream) != torch.cuda.current_stream(dev).cuda_stream:
        t.record_stream(torch.cuda.ExternalStream(int(stream), device=dev))
    return t


def _stream_of(dev, stream):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))


def _loss_pair(what, target, p):
    """the checks of one (target, p) pair -> (kind, n, M)"""
    kind = _kind(what, (("target", target), ("p", p)))
    ts, ps = tuple(target.shape), tuple(p.shape)
    if len(ts) != 2 or len(ps) != 2:
        raise RuntimeError(f"{what}: target and p must be [n, M] arrays, got shapes {ts} and {ps}")
    if ts != ps:
        raise RuntimeError(f"{what}: target and p must have one shape, got {ts} and {ps}")
    n, M = ts
    if M < 1 or M > MAX_ENTRIES:
        raise RuntimeError(f"{what}: M must be in [1, 2^20], got {M}")
    _check_rows(what, n)
    _check_dtype(what, "target", target, "float32")
    _check_dtype(what, "p", p, "float32")
    return kind, n, M


def _launch_loss(t, p, n, M, scale, out, stream):
    _call(lib.azmi_sample_loss(t.data_ptr(), p.data_ptr(), n, M, float(scale), out.data_ptr(), t.device.index, _stream_of(t.device, stream)))


def sample_loss(target, p, scale=1.0, device=0, stream=None):
    """loss[i] = -scale * sum over target[i, m] > 0 of target[i, m] * log(max(p[i, m], FLT_MIN)) for two [n, M] float32 arrays, in
    float64 (azmi_sample_loss): NNWrapper.sample_loss_pi at scale = 1 and sample_loss_v at scale = cv, on PROBABILITIES (what
    HipLeafNet writes) where the reference holds log-probabilities.  A zero target contributes exactly 0; a positive target on
    an underflowed probability stays finite.  -> float64 [n], numpy for numpy (staged on `device`), a CUDA tensor for CUDA tensors
    (enqueued on `stream`, a raw HIP stream handle, default the current one; no synchronisation; the inputs must be ready on that
    stream).  A negative target is an error for numpy inputs; on the
    device path it makes the row NaN, which resample_plan reports.  n == 0 touches no device."""
    what = "sample_loss"
    kind, n, M = _loss_pair(what, target, p)
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        raise RuntimeError(f"{what}: scale must be a number, got {scale!r}") from None
    if not np.isfinite(scale):
        raise RuntimeError(f"{what}: scale must be finite, got {scale!r}")
    if kind == "numpy":
        device = _check_device(what, device)
        if n and (target < 0).any():
            i, m = np.argwhere(target < 0)[0]
            raise RuntimeError(f"{what}: a negative target: target[{i}, {m}] = {target[i, m]!r}")
        if n == 0:
            return np.zeros(0, np.float64)
        t, q = _stage(target, device), _stage(p, device)
    else:
        t, q = target, p
    import torch
    out = _empty(n, torch.float64, t.device, stream)
    if n:
        _launch_loss(t, q, n, M, scale, out, stream)
    return out.cpu().numpy() if kind == "numpy" else out


def _plan(loss_t, seed, copies_t, offsets_t, stream):
    """azmi_resample_plan on a float64 CUDA tensor -> the record (copies_t / offsets_t None: the sums alone)"""
    rec = ResampleRecordC()
    _call(lib.azmi_resample_plan(loss_t.data_ptr(), int(loss_t.shape[0]), seed, None if copies_t is None else copies_t.data_ptr(),
                                 None if offsets_t is None else offsets_t.data_ptr(), C.byref(rec), loss_t.device.index,
                                 _stream_of(loss_t.device, stream)))
    return rec


def resample_plan(loss, seed, device=0, stream=None):
    """The copy count of every sample from its share of the total loss (azmi_resample_plan; game_runner.py:1183-1193):
    total_loss <= 0 gives every sample one copy, otherwise, in float64,

        w = 0.5 + (loss[i] / total_loss) * 0.5 * n,  k = floor(w),  copies[i] = k + (u_i < w - k)
        u_i = (mix64(seed + 0x9E3779B97F4A7C15 * (i + 1)) >> 11) * 2^-53

    (the draw is this package's: the reference's comes from the global numpy state).  `loss`: float64 [n].
    -> (copies, offsets, rows_out, total_loss): copies [n] uint32, offsets [n] uint64 = the exclusive prefix sum of copies (CUDA
    tensors: int32 / int64 with the same bits), rows_out = their sum, total_loss a float whose bits depend on the losses alone.
    One synchronisation.  Raises RuntimeError naming the first row when a loss is NaN or infinite.  n == 0 touches no device."""
    what = "resample_plan"
    kind = _kind(what, (("loss", loss),))
    if len(loss.shape) != 1:
        raise RuntimeError(f"{what}: loss must be one-dimensional, got shape {tuple(loss.shape)}")
    n = int(loss.shape[0])
    _check_rows(what, n)
    _check_dtype(what, "loss", loss, "float64")
    seed = _check_seed(what, seed)
    if kind == "numpy":
        device = _check_device(what, device)
        if n == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0, 0.0
        loss_t = _stage(loss, device)
    else:
        loss_t = loss
    import torch
    copies = _empty(n, torch.int32, loss_t.device, stream)
    offsets = _empty(n, torch.int64, loss_t.device, stream)
    if n == 0:
        return copies, offsets, 0, 0.0
    rec = _plan(loss_t, seed, copies, offsets, stream)
    if rec.nonfinite:
        raise RuntimeError(f"{what}: {rec.nonfinite} of {n} losses are not finite, the first at row {rec.first_nonfinite} (first_nonfinite)")
    if kind == "numpy":
        return copies.cpu().numpy().view(np.uint32), offsets.cpu().numpy().view(np.uint64), int(rec.rows_out), float(rec.total_loss)
    return copies, offsets, int(rec.rows_out), float(rec.total_loss)


def _gather(copies_t, offsets_t, n, rows_out, arrays_t, stream):
    """azmi_resample_gather on CUDA tensors -> the output tensors"""
    outs = [_empty((rows_out,) + tuple(x.shape[1:]), x.dtype, x.device, stream) for x in arrays_t]
    if n == 0 or rows_out == 0:
        return outs
    # one launch per array: measured faster than one launch over all three (the grid of a joint launch is sized for the array with
    # the widest lane groups, and the narrow arrays' surplus workgroups only start and leave)
    for x, o in zip(arrays_t, outs):
        ins, dst = (C.c_void_p * 1)(x.data_ptr()), (C.c_void_p * 1)(o.data_ptr())
        rb = (C.c_uint32 * 1)(int(np.prod(x.shape[1:], dtype=np.int64)) * x.element_size())
        _call(lib.azmi_resample_gather(copies_t.data_ptr(), offsets_t.data_ptr(), n, 1, ins, dst, rb, copies_t.device.index,
                                       _stream_of(copies_t.device, stream)))
    return outs


def _check_row_arrays(what, n, named):
    for name, x in named:
        shape = tuple(x.shape)
        if len(shape) < 1 or shape[0] != n:
            raise RuntimeError(f"{what}: {name} must hold one row per sample ({n}), got shape {shape}")
        _check_dtype(what, name, x, "float32")
        row = int(np.prod(shape[1:], dtype=np.int64))
        if row < 1 or row * 4 >= 1 << 32:
            raise RuntimeError(f"{what}: {name}: a row of {row} elements: rows hold 1 to 2^30 - 1 float32")


def resample_rows(copies, offsets, *arrays, rows_out=None, device=0, stream=None):
    """out[offsets[i] + c] = x[i] for c < copies[i], for every row array x ([n, ...] float32): x[np.repeat(np.arange(n), copies)]
    one launch per array (azmi_resample_gather).  copies / offsets as resample_plan returns them; `rows_out` (their
    sum) saves CUDA-tensor callers the synchronisation that reading it back costs.  -> the list of gathered arrays."""
    what = "resample_rows"
    named = [(f"arrays[{k}]", x) for k, x in enumerate(arrays)]
    kind = _kind(what, [("copies", copies), ("offsets", offsets)] + named)
    if len(copies.shape) != 1 or tuple(offsets.shape) != tuple(copies.shape):
        raise RuntimeError(f"{what}: copies and offsets must be one-dimensional and of one length, got shapes {tuple(copies.shape)} and {tuple(offsets.shape)}")
    n = int(copies.shape[0])
    _check_rows(what, n)
    _check_dtype(what, "copies", copies, ("uint32", "int32"))
    _check_dtype(what, "offsets", offsets, ("uint64", "int64"))
    _check_row_arrays(what, n, named)
    if rows_out is not None and (isinstance(rows_out, bool) or not isinstance(rows_out, (int, np.integer)) or rows_out < 0):
        raise RuntimeError(f"{what}: rows_out must be a row count, got {rows_out!r}")
    if kind == "numpy":
        device = _check_device(what, device)
        total = int(copies.sum(dtype=np.uint64)) if rows_out is None else int(rows_out)
        if n == 0 or total == 0 or not arrays:
            return [np.zeros((total,) + x.shape[1:], np.float32) for x in arrays]
        outs = _gather(_stage(copies.view(np.int32), device), _stage(offsets.view(np.int64), device), n, total,
                       [_stage(x, device) for x in arrays], stream)
        return [o.cpu().numpy() for o in outs]
    total = int(copies.sum().item()) if rows_out is None else int(rows_out)
    return _gather(copies, offsets, n, total, list(arrays), stream)


def _check_samples(what, samples, batch_rows):
    """-> (kind, n, canonical [n, C, H, W], v [n, V], pi [n, M]): the triple of self_play() or of symmetries_batch()"""
    try:
        canonical, v, pi = samples
    except (TypeError, ValueError):
        raise RuntimeError(f"{what}: samples must be the (canonical, v, pi) triple") from None
    named = (("canonical", canonical), ("v", v), ("pi", pi))
    kind = _kind(what, named)
    if isinstance(batch_rows, bool) or not isinstance(batch_rows, (int, np.integer)) or batch_rows < 1:
        raise RuntimeError(f"{what}: batch_rows must be an integer >= 1, got {batch_rows!r}")
    cs, vs, ps = tuple(canonical.shape), tuple(v.shape), tuple(pi.shape)
    if len(cs) < 4 or len(vs) != len(cs) - 2 or len(ps) != len(cs) - 2 or cs[:-3] != vs[:-1] or cs[:-3] != ps[:-1]:
        raise RuntimeError(f"{what}: the shapes of canonical [n, C, H, W], v [n, V] and pi [n, M] (or [n, NS, ...] each) do not agree: "
                           f"{cs}, {vs}, {ps}")
    n = int(np.prod(cs[:-3], dtype=np.int64))
    _check_rows(what, n)
    if not 1 <= ps[-1] <= MAX_ENTRIES or not 1 <= vs[-1] <= MAX_ENTRIES:
        raise RuntimeError(f"{what}: M must be in [1, 2^20], got pi rows of {ps[-1]} and v rows of {vs[-1]}")
    for name, x in named:
        _check_dtype(what, name, x, "float32")
    return kind, n, canonical.reshape((n,) + cs[-3:]), v.reshape(n, vs[-1]), pi.reshape(n, ps[-1])


def _net_losses(net, c, v, pi, n, batch_rows, cv, stream):
    """the net over the samples in chunks of batch_rows into one reused scratch, k_sample_loss on each chunk
    -> (pi loss [n], v loss [n] or None when cv is None), float64 CUDA tensors"""
    import torch
    B = max(1, min(int(batch_rows), n))
    v_s = _empty((B, v.shape[1]), torch.float32, c.device, stream)
    pi_s = _empty((B, pi.shape[1]), torch.float32, c.device, stream)
    st = torch.cuda.current_stream(c.device).cuda_stream if stream is None else int(stream)
    loss_pi = _empty(n, torch.float64, c.device, stream)
    loss_v = None if cv is None else _empty(n, torch.float64, c.device, stream)
    for lo in range(0, n, B):
        hi = min(n, lo + B)
        net.forward(c[lo:hi], v_s[:hi - lo], pi_s[:hi - lo], stream=st)
        _launch_loss(pi[lo:hi], pi_s[:hi - lo], hi - lo, int(pi.shape[1]), 1.0, loss_pi[lo:hi], st)
        if cv is not None:
            _launch_loss(v[lo:hi], v_s[:hi - lo], hi - lo, int(v.shape[1]), cv, loss_v[lo:hi], st)
    return loss_pi, loss_v


def resample_by_surprise(samples, net, seed, batch_rows=65536, data_folder=None, iteration=0, data_save_size=30_000, device=0, stream=None):
    """game_runner.resample_by_surprise on the device: the cross-entropy of `net` (a HipLeafNet) against every sample's policy
    target, a copy count per sample from its share of the total loss (resample_plan), the rows repeated that many times.
    `samples`: the (canonical, v, pi) triple of self_play() or of symmetries_batch() ([n, NS, ...] is read as n * NS rows).
    The net runs over chunks of `batch_rows` rows into one reused scratch.  -> ((canonical, v, pi) resampled, loss), loss the
    float64 per-sample array the reference returns for logging.  With `data_folder` the result is also written as the
    reference's `.ptz` triples, `data_save_size` rows per batch.  One host synchronisation: the plan's record.  The reference's
    file naming, checkpoint loading and clean-up stay with the caller."""
    what = "resample_by_surprise"
    kind, n, c, v, pi = _check_samples(what, samples, batch_rows)
    seed = _check_seed(what, seed)
    if not hasattr(net, "forward"):
        raise RuntimeError(f"{what}: net must be a HipLeafNet, got {type(net).__name__}")
    if kind == "numpy":
        device = _check_device(what, device)
        if n == 0:
            return (c.copy(), v.copy(), pi.copy()), np.zeros(0, np.float64)
        c, v, pi = _stage(c, device), _stage(v, device), _stage(pi, device)
    import torch
    if n == 0:
        return (c, v, pi), torch.empty(0, dtype=torch.float64, device=c.device)
    loss, _ = _net_losses(net, c, v, pi, n, batch_rows, None, stream)
    copies = _empty(n, torch.int32, c.device, stream)
    offsets = _empty(n, torch.int64, c.device, stream)
    rec = _plan(loss, seed, copies, offsets, stream)
    if rec.nonfinite:
        raise RuntimeError(f"{what}: {rec.nonfinite} of {n} sample losses are not finite, the first at row {rec.first_nonfinite} (first_nonfinite): "
                           "a NaN from the net, or a negative policy target")
    rows_out = int(rec.rows_out)
    out = tuple(_gather(copies, offsets, n, rows_out, [c, v, pi], stream))
    if data_folder is not None and rows_out:
        from . import history_io
        for b, lo in enumerate(range(0, rows_out, int(data_save_size))):
            hi = min(rows_out, lo + int(data_save_size))
            history_io.write_history_batch(data_folder, iteration, b, out[0][lo:hi], out[1][lo:hi], out[2][lo:hi])
    if kind == "numpy":
        return tuple(o.cpu().numpy() for o in out), loss.cpu().numpy()
    return out, loss


def iteration_losses(samples, net, cv=1.0, batch_rows=65536, device=0, stream=None):
    """(v_loss, pi_loss) of NNWrapper.losses (neural_net.py:644-661, 881-886): the means over the samples of the value loss
    (k_sample_loss at scale = cv on the value rows) and of the policy loss (scale = 1), float64 means through the plan's
    reduction (the reference: float32 batch means).  Raises RuntimeError naming the first row whose loss is NaN or infinite (a NaN
    from the net, a negative target).  No samples: (0.0, 0.0)."""
    what = "iteration_losses"
    kind, n, c, v, pi = _check_samples(what, samples, batch_rows)
    try:
        cv = float(cv)
    except (TypeError, ValueError):
        raise RuntimeError(f"{what}: cv must be a number, got {cv!r}") from None
    if not hasattr(net, "forward"):
        raise RuntimeError(f"{what}: net must be a HipLeafNet, got {type(net).__name__}")
    if n == 0:
        return 0.0, 0.0
    if kind == "numpy":
        device = _check_device(what, device)
        c, v, pi = _stage(c, device), _stage(v, device), _stage(pi, device)
    loss_pi, loss_v = _net_losses(net, c, v, pi, n, batch_rows, cv, stream)
    means = []
    for name, loss in (("value", loss_v), ("policy", loss_pi)):
        rec = _plan(loss, 0, None, None, stream)      # (the sums alone)
        if rec.nonfinite:
            raise RuntimeError(f"{what}: {rec.nonfinite} of {n} {name} losses are not finite, the first at row {rec.first_nonfinite} (first_nonfinite): "
                               "a NaN from the net, or a negative target")
        means.append(float(rec.total_loss) / n)
    return means[0], means[1]
