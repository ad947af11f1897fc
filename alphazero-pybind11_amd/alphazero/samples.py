"""The sample path between self-play and training, on the device (azmi_sample_loss / azmi_resample_plan / azmi_resample_gather,
csrc/samples_kernels.h): the reference's resample_by_surprise (game_runner.py:1148-1255) and the per-sample / per-iteration losses
behind it (NNWrapper.sample_loss, NNWrapper.losses, neural_net.py:644-676, 875-886), without the host round trip.

Every function takes numpy arrays (staged through the device) or CUDA tensors (in place, nothing leaves the device but the plan's
record) and answers in the kind it was given.  Argument errors are RuntimeErrors raised before any device call; inputs are
contiguous float32 (the losses: float64) and are never converted silently.  torch is imported inside the functions: importing
the package does not import it.

Second half (azmi_sample_metrics / azmi_sample_plane_argmax / azmi_sample_metrics_reduce, csrc/sample_metrics_kernels.h): the
per-row policy and value diagnostics of a net against the samples - sample_metrics, plane_argmax - and the two consumers the
reference has for them: eval_metrics (network_pareto.eval_loss, network_pareto.py:652-738) and analyze_samples
(game_runner._analyze_iteration_variants, game_runner.py:2509-2627).

Third part (azmi_samples_reservoir_keys / azmi_samples_select_top / azmi_samples_window_gather, csrc/samples_window_kernels.h): the
history window and the recency-weighted reservoir that training reads - reservoir_keys, select_top, window_batches and the
SampleWindow that holds them together (calc_hist_size, update_reservoir and train, game_runner.py:955-1008, 1701-1869, 1289-1345).

Fourth part (azmi_samples_feature_rank, csrc/feature_rank_kernels.h; azmi_net_trunk_features, csrc/leafnet_f32.hip): feature_rank, the
participation ratio of a feature matrix from its centred Gram matrix in float64, and effective_rank, NNWrapper.effective_rank
(neural_net.py:826-873) over the pooled trunk features of an fp32 HipLeafNet."""
import ctypes as C
import enum

import numpy as np

from . import _args, _rng
from ._capi import lib, ResampleRecordC, SampleMetricsRecordC, SelectRecordC, WINDOW_MAX_SEGMENTS, FeatureRankRecordC, FEATURE_RANK_MAX_CHANNELS

MAX_ROWS = 1 << 30
MAX_ENTRIES = 1 << 20
MAX_BUCKETS = 8
MAX_PLANES = 16
_GOLDEN = 0x9E3779B97F4A7C15


class Metric(enum.IntEnum):
    """the float64 columns of sample_metrics: enum SampleMetric of csrc/sample_metrics_kernels.h"""
    PI_LOSS = 0
    V_LOSS = 1
    TARGET_ENTROPY = 2
    ENTROPY = 3
    KL = 4
    TOP1 = 5
    NET_TOP1 = 6
    NET_AT_MCTS = 7
    TOP1_GAP = 8
    TOP1_AGREE = 9
    TOP3_OVERLAP = 10
    V_PRED = 11
    V_ACTUAL = 12


METRIC_COLUMNS = tuple(m.name.lower() for m in Metric)
INDEX_COLUMNS = ("mcts_argmax", "net_argmax")
# the ten per-sample arrays of _analyze_iteration_variants (game_runner.py:2602-2613)
ANALYSIS_KEYS = ("pi_loss", "v_loss", "entropy", "top1", "net_top1", "net_at_mcts", "top1_gap", "top1_agree", "v_pred", "v_actual")
# the keys of network_pareto.eval_loss, and the row count
EVAL_KEYS = ("v_loss", "v_loss_raw", "pi_loss", "total_loss", "top1_agree", "top3_agree", "kl_div", "target_entropy", "kl_gap", "count")


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
        device = _args.device_index(device, what)
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
    seed = _args.seed64(seed, what)
    if kind == "numpy":
        device = _args.device_index(device, what)
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
    if rows_out is not None:
        _args.integer(rows_out, f"{what}: rows_out must be a row count, got {rows_out!r}", 0)
    if kind == "numpy":
        device = _args.device_index(device, what)
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
    _args.integer(batch_rows, f"{what}: batch_rows must be an integer >= 1, got {batch_rows!r}", 1)
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
    seed = _args.seed64(seed, what)
    if not hasattr(net, "forward"):
        raise RuntimeError(f"{what}: net must be a HipLeafNet, got {type(net).__name__}")
    if kind == "numpy":
        device = _args.device_index(device, what)
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
        device = _args.device_index(device, what)
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


# ---- per-row diagnostics: sample_metrics, plane_argmax, eval_metrics, analyze_samples ------------------------------------------
def _check_cv(what, cv):
    try:
        cv = float(cv)
    except (TypeError, ValueError):
        raise RuntimeError(f"{what}: cv must be a number, got {cv!r}") from None
    if not np.isfinite(cv):
        raise RuntimeError(f"{what}: cv must be finite, got {cv!r}")
    return cv


def _check_index(what, name, x):
    return _args.integer(x, f"{what}: {name} must be an integer >= 0, got {x!r}", 0)


def _launch_metrics(t_pi, p_pi, t_v, p_v, n, cv, cols, lo, mcts, net, stream):
    """k_sample_metrics over n rows into the rows lo .. lo + n of the [13, N] float64 tensor `cols` and of the two index tensors"""
    _call(lib.azmi_sample_metrics(t_pi.data_ptr(), p_pi.data_ptr(), t_v.data_ptr(), p_v.data_ptr(), n, int(t_pi.shape[1]), int(t_v.shape[1]),
                                  cv, cols.data_ptr() + 8 * lo, int(cols.shape[1]), mcts.data_ptr() + 4 * lo, net.data_ptr() + 4 * lo,
                                  cols.device.index, _stream_of(cols.device, stream)))


def _metric_tensors(n, dev, stream):
    import torch
    return (_empty((len(Metric), n), torch.float64, dev, stream), _empty(n, torch.int32, dev, stream), _empty(n, torch.int32, dev, stream))


def sample_metrics(pi_target, pi_p, v_target, v_p, cv=1.0, device=0, stream=None):
    """The per-row diagnostics of a net's answers (pi_p [n, M], v_p [n, V]: PROBABILITIES, what HipLeafNet writes) against the samples'
    targets (pi_target [n, M], v_target [n, V]), one launch that reads every element once (azmi_sample_metrics), float64 on the
    float32 inputs.  -> {column: array [n]}: the thirteen float64 columns of Metric (METRIC_COLUMNS)

        pi_loss         -sum over t > 0 of t * log(max(p, FLT_MIN))       sample_loss(pi_target, pi_p), bit for bit
        v_loss          the same on the value rows at scale cv            sample_loss(v_target, v_p, scale=cv), bit for bit
        target_entropy  -sum over t > 0 of t * log(t)                     (network_pareto.py:716)
        entropy         -sum over all m of t * log(t + 1e-9)              (game_runner.py:2562)
        kl              sum over t > 0 of t * log(t / (p + 1e-10))        (network_pareto.py:713)
        top1, net_top1  max t, max p            net_at_mcts  p[mcts_argmax]            top1_gap  top1 - net_at_mcts
        top1_agree      1.0 when net_argmax == mcts_argmax, else 0.0
        top3_overlap    |top3(p) & top3(t)|, 0..3 (M < 3: the sets have M members)
        v_pred, v_actual  v_p[:, 0], v_target[:, 0]

    and the uint32 columns mcts_argmax and net_argmax (CUDA tensors: int32 with the same bits).  Ties in every argmax and top-3
    go to the LOWER index (np.argmax; the first three of np.argsort(-x, kind="stable"); pib.max(dim=1) on the reference's CPU path) -
    unlike policy_divergences and sweep_metrics, where the higher index wins as in policy_metrics.py.  A negative target is NOT
    an error here, on either path: it makes the sums of its row NaN (pi_loss, target_entropy, entropy, kl; v_loss for a value
    target); a NaN probability makes NaN what reads it (pi_loss and kl under a positive target, net_top1, net_at_mcts and top1_gap at
    the target's argmax); the index columns of such a row are unspecified but < M.  numpy arrays are staged on `device`; CUDA
    tensors are used in place on `stream` with no synchronisation (the columns are the rows of one [13, n] tensor).  n == 0 touches
    no device."""
    what = "sample_metrics"
    named = (("pi_target", pi_target), ("pi_p", pi_p), ("v_target", v_target), ("v_p", v_p))
    kind = _kind(what, named)
    shapes = [tuple(x.shape) for _, x in named]
    if any(len(s) != 2 for s in shapes):
        raise RuntimeError(f"{what}: pi_target and pi_p must be [n, M] arrays, v_target and v_p [n, V] arrays, got shapes "
                           + ", ".join(str(s) for s in shapes))
    if shapes[0] != shapes[1]:
        raise RuntimeError(f"{what}: pi_target and pi_p must have one shape, got {shapes[0]} and {shapes[1]}")
    if shapes[2] != shapes[3]:
        raise RuntimeError(f"{what}: v_target and v_p must have one shape, got {shapes[2]} and {shapes[3]}")
    if shapes[0][0] != shapes[2][0]:
        raise RuntimeError(f"{what}: the policy and the value arrays must hold one row per sample, got {shapes[0][0]} and {shapes[2][0]} rows")
    (n, M), V = shapes[0], shapes[2][1]
    if not 1 <= M <= MAX_ENTRIES or not 1 <= V <= MAX_ENTRIES:
        raise RuntimeError(f"{what}: M and V must be in [1, 2^20], got M = {M} and V = {V}")
    _check_rows(what, n)
    for name, x in named:
        _check_dtype(what, name, x, "float32")
    cv = _check_cv(what, cv)
    if kind == "numpy":
        device = _args.device_index(device, what)
        if n == 0:
            out = {name: np.zeros(0, np.float64) for name in METRIC_COLUMNS}
            out.update({name: np.zeros(0, np.uint32) for name in INDEX_COLUMNS})
            return out
        pi_target, pi_p, v_target, v_p = (_stage(x, device) for _, x in named)
    cols, mcts, net = _metric_tensors(n, pi_target.device, stream)
    if n:
        _launch_metrics(pi_target, pi_p, v_target, v_p, n, cv, cols, 0, mcts, net, stream)
    if kind == "numpy":
        host = cols.cpu().numpy()
        out = {name: host[k] for k, name in enumerate(METRIC_COLUMNS)}
        out["mcts_argmax"], out["net_argmax"] = mcts.cpu().numpy().view(np.uint32), net.cpu().numpy().view(np.uint32)
        return out
    out = {name: cols[k] for k, name in enumerate(METRIC_COLUMNS)}
    out["mcts_argmax"], out["net_argmax"] = mcts, net
    return out


def plane_argmax(canonical, first_plane, n_planes, row, col, device=0, stream=None):
    """The lower-index argmax over the planes first_plane .. first_plane + n_planes - 1 (1 to 16 planes) of canonical [n, C, H, W] at
    the cell (row, col) (azmi_sample_plane_argmax): canonical[:, first_plane:first_plane + n_planes, row, col].argmax(1).
    -> uint8 [n], numpy for numpy (staged on `device`), a CUDA tensor for a CUDA tensor (on `stream`, no synchronisation).
    [n, NS, C, H, W] is read as n * NS rows.  plane_argmax(canonical, 32, 4, 6, 6) is the variant id of the unified StarGambit
    encoding (game_runner.py:2535)."""
    what = "plane_argmax"
    kind = _kind(what, (("canonical", canonical),))
    shape = tuple(canonical.shape)
    if len(shape) < 4:
        raise RuntimeError(f"{what}: canonical must be an [n, C, H, W] array, got shape {shape}")
    n = int(np.prod(shape[:-3], dtype=np.int64))
    Cn, H, W = shape[-3:]
    _check_rows(what, n)
    if min(Cn, H, W) < 1 or Cn * H * W >= 1 << 30:
        raise RuntimeError(f"{what}: canonical: a row of {Cn} x {H} x {W}: rows hold 1 to 2^30 - 1 float32")
    _check_dtype(what, "canonical", canonical, "float32")
    first_plane, n_planes = _check_index(what, "first_plane", first_plane), _check_index(what, "n_planes", n_planes)
    row, col = _check_index(what, "row", row), _check_index(what, "col", col)
    if not 1 <= n_planes <= MAX_PLANES:
        raise RuntimeError(f"{what}: n_planes must be in [1, {MAX_PLANES}], got {n_planes}")
    if first_plane + n_planes > Cn:
        raise RuntimeError(f"{what}: the planes {first_plane} .. {first_plane + n_planes - 1} are outside the {Cn} planes of canonical")
    if row >= H or col >= W:
        raise RuntimeError(f"{what}: the cell ({row}, {col}) is outside the {H} x {W} board")
    if kind == "numpy":
        device = _args.device_index(device, what)
        if n == 0:
            return np.zeros(0, np.uint8)
        canonical = _stage(canonical, device)
    import torch
    out = _empty(n, torch.uint8, canonical.device, stream)
    if n:
        _call(lib.azmi_sample_plane_argmax(canonical.data_ptr(), n, Cn, H, W, first_plane, n_planes, row, col, out.data_ptr(),
                                           canonical.device.index, _stream_of(canonical.device, stream)))
    return out.cpu().numpy() if kind == "numpy" else out


def _check_buckets(what, sample_arrays, n, buckets, n_buckets, names):
    """-> (n_buckets or None without buckets, names)"""
    if buckets is None:
        if n_buckets is not None or names is not None:
            raise RuntimeError(f"{what}: n_buckets and names go with buckets, which is None")
        return None, None
    _kind(what, tuple(sample_arrays) + (("buckets", buckets),))
    if len(buckets.shape) != 1 or int(buckets.shape[0]) != n:
        raise RuntimeError(f"{what}: buckets must hold one id per sample ({n}), got shape {tuple(buckets.shape)}")
    _check_dtype(what, "buckets", buckets, "uint8")
    if names is not None:
        names = list(names)
        if any(not isinstance(x, str) for x in names) or len(set(names)) != len(names) or "overall" in names:
            raise RuntimeError(f'{what}: names must be distinct strings other than "overall", got {names!r}')
    if n_buckets is None:
        if names is None:
            raise RuntimeError(f"{what}: with buckets, give n_buckets or names")
        n_buckets = len(names)
    n_buckets = _args.integer(n_buckets, f"{what}: n_buckets must be an integer in [1, {MAX_BUCKETS}], got {n_buckets!r}", 1, MAX_BUCKETS)
    if names is None:
        names = [str(b) for b in range(n_buckets)]
    if len(names) != n_buckets:
        raise RuntimeError(f"{what}: {len(names)} names for {n_buckets} buckets")
    return n_buckets, names


def _net_metrics(net, c, v, pi, n, batch_rows, cv, stream):
    """the net over the samples in chunks of batch_rows into one reused scratch (as _net_losses), one k_sample_metrics launch per chunk
    -> (columns [13, n] float64, mcts_argmax [n], net_argmax [n] int32), CUDA tensors"""
    import torch
    B = max(1, min(int(batch_rows), n))
    v_s = _empty((B, v.shape[1]), torch.float32, c.device, stream)
    pi_s = _empty((B, pi.shape[1]), torch.float32, c.device, stream)
    st = torch.cuda.current_stream(c.device).cuda_stream if stream is None else int(stream)
    cols, mcts, net_idx = _metric_tensors(n, c.device, stream)
    for lo in range(0, n, B):
        hi = min(n, lo + B)
        net.forward(c[lo:hi], v_s[:hi - lo], pi_s[:hi - lo], stream=st)
        _launch_metrics(pi[lo:hi], pi_s[:hi - lo], v[lo:hi], v_s[:hi - lo], hi - lo, cv, cols, lo, mcts, net_idx, st)
    return cols, mcts, net_idx


def _reduce(cols, n, buckets_t, n_buckets, stream):
    """azmi_sample_metrics_reduce on the [13, N] columns -> the record"""
    rec = SampleMetricsRecordC()
    _call(lib.azmi_sample_metrics_reduce(cols.data_ptr(), int(cols.shape[1]), n, None if buckets_t is None else buckets_t.data_ptr(),
                                         1 if buckets_t is None else n_buckets, C.byref(rec), cols.device.index, _stream_of(cols.device, stream)))
    return rec


def _eval_dict(sums, count, cv):
    """the figures of network_pareto.eval_loss (network_pareto.py:720-738) from the column sums of `count` rows"""
    if count == 0:
        return dict({k: float("nan") for k in EVAL_KEYS}, count=0)
    mean = lambda m: float(sums[m]) / count
    v_loss, pi_loss, target_entropy = mean(Metric.V_LOSS), mean(Metric.PI_LOSS), mean(Metric.TARGET_ENTROPY)
    return {"v_loss": v_loss, "v_loss_raw": v_loss / cv if cv else float("nan"), "pi_loss": pi_loss, "total_loss": v_loss + pi_loss,
            "top1_agree": mean(Metric.TOP1_AGREE), "top3_agree": float(sums[Metric.TOP3_OVERLAP]) / (3 * count), "kl_div": mean(Metric.KL),
            "target_entropy": target_entropy, "kl_gap": pi_loss - target_entropy, "count": int(count)}


def eval_metrics(samples, net, cv=1.0, batch_rows=65536, buckets=None, n_buckets=None, names=None, device=0, stream=None):
    """network_pareto.eval_loss (network_pareto.py:652-738) on the device: the held-out metric set of `net` (a HipLeafNet) over
    `samples` (the (canonical, v, pi) triple of self_play() or of symmetries_batch()).  The net runs over chunks of `batch_rows` rows
    into one reused scratch, one k_sample_metrics launch per chunk writes the [13, n] columns, one bucketed reduction sums them.
    -> {"v_loss", "v_loss_raw" (= v_loss / cv), "pi_loss", "total_loss", "top1_agree", "top3_agree" (= sum of top3_overlap / (3 n)),
    "kl_div", "target_entropy", "kl_gap" (= pi_loss - target_entropy), "count"}.  With `buckets` (uint8 [n], ids below `n_buckets`
    <= 8, default len(names); `names` default "0", "1", ...): {name: that dict} over the non-empty buckets, and "overall".
    The means are float64 per-sample means; the reference takes the mean of float32 batch means, the same figure when all batches
    have one size.  No AMP: the net's own precision tier decides.  One host synchronisation, the reduction's record.  Raises
    RuntimeError naming the first row whose loss, entropy or kl is NaN or infinite, and when a bucket id is >= n_buckets.  No samples:
    every figure is NaN and count is 0."""
    what = "eval_metrics"
    kind, n, c, v, pi = _check_samples(what, samples, batch_rows)
    cv = _check_cv(what, cv)
    if not hasattr(net, "forward"):
        raise RuntimeError(f"{what}: net must be a HipLeafNet, got {type(net).__name__}")
    B, names = _check_buckets(what, (("canonical", c), ("v", v), ("pi", pi)), n, buckets, n_buckets, names)
    if kind == "numpy":
        device = _args.device_index(device, what)
    if n == 0:
        return _eval_dict(None, 0, cv) if B is None else {"overall": _eval_dict(None, 0, cv)}
    if kind == "numpy":
        c, v, pi = _stage(c, device), _stage(v, device), _stage(pi, device)
        buckets = None if B is None else _stage(buckets, device)
    cols, _, _ = _net_metrics(net, c, v, pi, n, batch_rows, cv, stream)
    rec = _reduce(cols, n, buckets, B, stream)
    if rec.nonfinite:
        raise RuntimeError(f"{what}: {rec.nonfinite} of {n} samples have a loss, entropy or kl that is not finite, the first at row "
                           f"{rec.first_nonfinite} (first_nonfinite): a NaN from the net, or a negative target")
    if rec.invalid:
        raise RuntimeError(f"{what}: {rec.invalid} of {n} bucket ids are >= n_buckets = {B}")
    overall = _eval_dict(rec.total, n, cv)
    if B is None:
        return overall
    out = {names[b]: _eval_dict(rec.sum[b], rec.count[b], cv) for b in range(B) if rec.count[b]}
    out["overall"] = overall
    return out


def analyze_samples(samples, net, cv=1.0, batch_rows=65536, buckets=None, names=None, device=0, stream=None):
    """game_runner._analyze_iteration_variants (game_runner.py:2509-2627) on the device: the per-sample arrays "pi_loss", "v_loss",
    "entropy", "top1", "net_top1", "net_at_mcts", "top1_gap", "top1_agree", "v_pred", "v_actual" of `net` over `samples` (float64 columns
    of sample_metrics), split by bucket.  -> {"overall": {key: array [n]}} without `buckets`; with `buckets` (uint8 [n]) and `names`
    (default "0", "1", ... up to the largest id) {name: {key: array of the bucket's rows}} over the non-empty buckets, as the
    reference returns per variant.  numpy samples give numpy arrays, CUDA tensors give CUDA tensors.  The split is boolean-mask
    indexing (it synchronises); the reference's sample loading and checkpoint loading stay with the caller."""
    what = "analyze_samples"
    kind, n, c, v, pi = _check_samples(what, samples, batch_rows)
    cv = _check_cv(what, cv)
    if not hasattr(net, "forward"):
        raise RuntimeError(f"{what}: net must be a HipLeafNet, got {type(net).__name__}")
    if buckets is None and names is not None:
        raise RuntimeError(f"{what}: names go with buckets, which is None")
    if buckets is not None:
        _kind(what, (("canonical", c), ("v", v), ("pi", pi), ("buckets", buckets)))
        if len(buckets.shape) != 1 or int(buckets.shape[0]) != n:
            raise RuntimeError(f"{what}: buckets must hold one id per sample ({n}), got shape {tuple(buckets.shape)}")
        _check_dtype(what, "buckets", buckets, "uint8")
        if names is not None:
            names = list(names)
            if any(not isinstance(x, str) for x in names) or len(set(names)) != len(names):
                raise RuntimeError(f"{what}: names must be distinct strings, got {names!r}")
    if kind == "numpy":
        device = _args.device_index(device, what)
    if n == 0:
        empty = {k: np.zeros(0, np.float64) for k in ANALYSIS_KEYS} if kind == "numpy" else None
        if empty is None:
            import torch
            empty = {k: torch.empty(0, dtype=torch.float64, device=c.device) for k in ANALYSIS_KEYS}
        return {"overall": empty} if buckets is None else {}
    if kind == "numpy":
        c, v, pi = _stage(c, device), _stage(v, device), _stage(pi, device)
    cols, _, _ = _net_metrics(net, c, v, pi, n, batch_rows, cv, stream)
    if stream is not None:
        import torch
        torch.cuda.ExternalStream(int(stream), device=cols.device).synchronize()      # the indexing below runs on the current stream
    if kind == "numpy":
        cols = cols.cpu().numpy()
    if buckets is None:
        return {"overall": {k: cols[Metric[k.upper()]] for k in ANALYSIS_KEYS}}
    top = int(buckets.max()) + 1
    if names is None:
        names = [str(b) for b in range(top)]
    if top > len(names):
        raise RuntimeError(f"{what}: a bucket id {top - 1} with {len(names)} names")
    out = {}
    for b, name in enumerate(names):
        mask = buckets == b
        if not bool(mask.any()):
            continue
        out[name] = {k: cols[Metric[k.upper()]][mask] for k in ANALYSIS_KEYS}
    return out


# ---- the history window and the reservoir: reservoir_keys, select_top, window_batches, SampleWindow ---------------------------------
def _check_vector(what, name, x, want):
    if len(x.shape) != 1:
        raise RuntimeError(f"{what}: {name} must be one-dimensional, got shape {tuple(x.shape)}")
    _check_rows(what, int(x.shape[0]))
    _check_dtype(what, name, x, want)
    return int(x.shape[0])


def reservoir_keys(iters, iteration, decay, seed, row_ids=None, with_bits=False, device=0, stream=None):
    """The keys of a weighted sample without replacement (azmi_samples_reservoir_keys; the weights of game_runner.py:1845-1846):

        key_i = log(u_i) / w_i,   w_i = decay ** max(0, iteration - iters[i])
        u_i = m_i * 2^-53,   m_i = ((mix64(seed + 0x9E3779B97F4A7C15 * (id_i + 1)) >> 12) << 1) | 1

    `iters`: int32 [n], the iteration every row came from; id_i = row_ids[i] (uint64 / int64 [n]) or i.  The k largest keys
    (select_top) draw k rows with the distribution of torch.multinomial(w, k, replacement=False), not with its stream.  A weight
    that underflows to 0 gives -inf.  -> float64 [n] (with_bits: (keys, m) with m uint64 / int64 [n]), numpy for numpy (staged on
    `device`), CUDA tensors for CUDA tensors (on `stream`, no synchronisation).  n == 0 touches no device."""
    what = "reservoir_keys"
    named = [("iters", iters)] + ([] if row_ids is None else [("row_ids", row_ids)])
    kind = _kind(what, named)
    n = _check_vector(what, "iters", iters, "int32")
    if row_ids is not None and (_check_vector(what, "row_ids", row_ids, ("uint64", "int64")) != n):
        raise RuntimeError(f"{what}: row_ids must hold one id per row ({n}), got shape {tuple(row_ids.shape)}")
    iteration = _args.number(iteration, f"{what}: iteration must be a finite number >= 0, got {iteration!r}")
    decay = _args.unit_fraction(decay, f"{what}: decay must be a number in (0, 1], got {decay!r}")
    seed = _args.seed64(seed, what)
    if kind == "numpy":
        device = _args.device_index(device, what)
        if n == 0:
            return (np.zeros(0, np.float64), np.zeros(0, np.uint64)) if with_bits else np.zeros(0, np.float64)
        iters = _stage(iters, device)
        row_ids = None if row_ids is None else _stage(row_ids.view(np.int64), device)
    import torch
    keys = _empty(n, torch.float64, iters.device, stream)
    bits = _empty(n, torch.int64, iters.device, stream) if with_bits else None
    if n:
        _call(lib.azmi_samples_reservoir_keys(iters.data_ptr(), None if row_ids is None else row_ids.data_ptr(), n, iteration, decay, seed,
                                              keys.data_ptr(), None if bits is None else bits.data_ptr(), iters.device.index,
                                              _stream_of(iters.device, stream)))
    if kind == "numpy":
        keys = keys.cpu().numpy()
        return (keys, bits.cpu().numpy().view(np.uint64)) if with_bits else keys
    return (keys, bits) if with_bits else keys


def select_top(keys, k, device=0, stream=None):
    """The rows of the k largest of the float64 `keys` [n], in ASCENDING ROW ORDER (azmi_samples_select_top): among equal keys the
    lower rows win, -0.0 counts as +0.0, -inf loses to every finite key: np.sort(np.argsort(-keys, kind="stable")[:k]).  A radix
    select and an ordered compaction on the device, no sort; the result does not depend on scheduling.
    -> (index int64 [k], {"selected": k, "threshold_key": the smallest chosen key, "first_bad_row": None}).  One synchronisation,
    the record.  Raises RuntimeError naming the first row whose key is NaN.  k == 0 touches no device."""
    what = "select_top"
    kind = _kind(what, (("keys", keys),))
    n = _check_vector(what, "keys", keys, "float64")
    k = _args.integer(k, f"{what}: k must be an integer in [0, n = {n}], got {k!r}", 0, n)
    if kind == "numpy":
        device = _args.device_index(device, what)
        if k == 0:
            return np.zeros(0, np.int64), {"selected": 0, "threshold_key": None, "first_bad_row": None}
        keys = _stage(keys, device)
    import torch
    index = _empty(k, torch.int64, keys.device, stream)
    if k == 0:
        return index, {"selected": 0, "threshold_key": None, "first_bad_row": None}
    rec = SelectRecordC()
    _call(lib.azmi_samples_select_top(keys.data_ptr(), n, k, index.data_ptr(), C.byref(rec), keys.device.index, _stream_of(keys.device, stream)))
    if rec.nan_rows:
        raise RuntimeError(f"{what}: {rec.nan_rows} of {n} keys are NaN, the first at row {rec.first_bad_row} (first_bad_row)")
    record = {"selected": int(rec.selected), "threshold_key": float(rec.threshold_key), "first_bad_row": None}
    return (index.cpu().numpy() if kind == "numpy" else index), record


def _row_shapes(what, c, v, pi):
    return tuple(c.shape[1:]), tuple(v.shape[1:]), tuple(pi.shape[1:])


def _check_segments(what, segments):
    """the checks of a window: a sequence of at most 64 (canonical, v, pi) triples of one kind, one device and one row shape
    -> (kind, [(canonical [n, C, H, W], v [n, V], pi [n, M])], [n])"""
    try:
        segments = list(segments)
    except TypeError:
        raise RuntimeError(f"{what}: segments must be a sequence of (canonical, v, pi) triples, got {type(segments).__name__}") from None
    if len(segments) > WINDOW_MAX_SEGMENTS:
        raise RuntimeError(f"{what}: at most {WINDOW_MAX_SEGMENTS} segments, got {len(segments)}")
    kinds, out, rows, shapes, named_all = set(), [], [], None, []
    for s, seg in enumerate(segments):
        try:
            canonical, v, pi = seg
        except (TypeError, ValueError):
            raise RuntimeError(f"{what}: segments[{s}] must be the (canonical, v, pi) triple") from None
        named = ((f"segments[{s}].canonical", canonical), (f"segments[{s}].v", v), (f"segments[{s}].pi", pi))
        named_all.extend(named)
        kinds.add(_kind(what, named))
        cs, vs, ps = tuple(canonical.shape), tuple(v.shape), tuple(pi.shape)
        if len(cs) != 4 or len(vs) != 2 or len(ps) != 2:
            raise RuntimeError(f"{what}: segments[{s}]: canonical [n, C, H, W], v [n, V] and pi [n, M] are wanted, got shapes {cs}, {vs}, {ps}")
        if not cs[0] == vs[0] == ps[0]:
            raise RuntimeError(f"{what}: segments[{s}]: canonical, v and pi must hold one row per sample, got {cs[0]}, {vs[0]} and {ps[0]} rows")
        _check_rows(what, cs[0])
        for name, x in named:
            _check_dtype(what, name, x, "float32")
            row = int(np.prod(x.shape[1:], dtype=np.int64))
            if row < 1 or row * 4 >= 1 << 26:
                raise RuntimeError(f"{what}: {name}: a row of {row} elements: rows hold 1 to 2^24 - 1 float32")
        if shapes is None:
            shapes = (cs[1:], vs[1:], ps[1:])
        elif shapes != (cs[1:], vs[1:], ps[1:]):
            raise RuntimeError(f"{what}: segments[{s}]: rows of shapes {cs[1:]}, {vs[1:]}, {ps[1:]} in a window of {shapes[0]}, {shapes[1]}, {shapes[2]}")
        out.append((canonical, v, pi))
        rows.append(int(cs[0]))
    if len(kinds) > 1:
        raise RuntimeError(f"{what}: numpy arrays and tensors are mixed among the segments")
    kind = kinds.pop() if kinds else "numpy"
    if kind == "torch" and len({str(x.device) for _, x in named_all}) > 1:
        raise RuntimeError(f"{what}: the segments are on different devices")
    return kind, out, rows


def _window_gather(arrays_t, rows_list, index_t, seed, pass_index, first, rows, stream):
    """azmi_samples_window_gather over the segments `arrays_t` of one row array -> the gathered tensor [rows, ...]"""
    x0 = arrays_t[0]
    out = _empty((rows,) + tuple(x0.shape[1:]), x0.dtype, x0.device, stream)
    if rows == 0:
        return out
    ns = len(arrays_t)
    ptrs = (C.c_void_p * ns)(*[x.data_ptr() if n else None for x, n in zip(arrays_t, rows_list)])
    counts = (C.c_uint64 * ns)(*rows_list)
    row_bytes = int(np.prod(x0.shape[1:], dtype=np.int64)) * x0.element_size()
    _call(lib.azmi_samples_window_gather(ptrs, counts, ns, row_bytes, None if index_t is None else index_t.data_ptr(), seed, pass_index, first,
                                         rows, out.data_ptr(), x0.device.index, _stream_of(x0.device, stream)))
    return out


def _pass_batches(segs_t, rows_list, batch_rows, seed, pass_index, first, batches, stream):
    """the batches of one pass over CUDA segments: one launch per array and batch, no synchronisation"""
    total, b = sum(rows_list), 0
    while first < total and (batches is None or b < batches):
        rows = min(batch_rows, total - first)
        yield tuple(_window_gather([seg[a] for seg in segs_t], rows_list, None, seed, pass_index, first, rows, stream) for a in range(3))
        first += rows
        b += 1


def window_batches(segments, batch_rows, seed, pass_index=0, first=0, batches=None, device=0, stream=None):
    """One shuffled pass over a window of samples, cut into training batches that mix the segments (azmi_samples_window_gather; the
    pass of StreamingCompressedDataset that train() consumes, game_runner.py:1289-1345, 1923-2009).  `segments`: up to 64
    (canonical, v, pi) triples, one per iteration, read as their concatenation of `total` rows.  Batch b holds the rows
    perm(first + b * batch_rows + j), j < batch_rows, perm the bijection of [0, total) keyed by (seed, pass_index) that DESIGN.md
    8.5.2 states; the last batch of the pass is short.  `batches`: stop after that many (None: the whole pass from `first`).
    -> a generator of (canonical, v, pi) batches, numpy for numpy (the segments are staged on `device` once), CUDA tensors for CUDA
    tensors (on `stream`): one launch per array and batch, no synchronisation.  The arguments are checked at the call, not at the
    first batch."""
    what = "window_batches"
    kind, segs, rows_list = _check_segments(what, segments)
    batch_rows = _args.integer(batch_rows, f"{what}: batch_rows must be an integer in [1, 2^30], got {batch_rows!r}", 1, MAX_ROWS)
    seed = _args.seed64(seed, what)
    pass_index = _args.integer(pass_index, f"{what}: pass_index must be an integer in [0, 2^63), got {pass_index!r}", 0, (1 << 63) - 1)
    total = sum(rows_list)
    first = _args.integer(first, f"{what}: first must be a row of the window, an integer in [0, {total}], got {first!r}", 0, total)
    if batches is not None:
        batches = _args.integer(batches, f"{what}: batches must be None or an integer >= 0, got {batches!r}", 0)
    if kind == "numpy":
        device = _args.device_index(device, what)

    def run():
        if first >= total or batches == 0:
            return
        segs_t = [tuple(_stage(x, device) for x in seg) for seg in segs] if kind == "numpy" else segs
        for batch in _pass_batches(segs_t, rows_list, batch_rows, seed, pass_index, first, batches, stream):
            yield tuple(x.cpu().numpy() for x in batch) if kind == "numpy" else batch
    return run()


class SampleWindow:
    """The history window and the recency-weighted reservoir of the reference's training loop, kept in HBM (calc_hist_size,
    game_runner.py:955-1008; update_reservoir, :1701-1869; train, :1289-1345): the last `hist_size` iterations as they were appended,
    the iterations that left the window in staging, and ONE reservoir chunk of at most `reservoir_rows` rows that update_reservoir
    merges the staging into with weights decay ** age.  The reference's n_chunks, chunks_per_update and file rotation bound host RAM
    and have no counterpart here.  Row ids are (iteration << 32) | row, the draw of an update is keyed by
    mix64(seed + 0x9E3779B97F4A7C15 * (iteration + 1)): a run is a function of `seed` and the samples."""

    def __init__(self, hist_size, reservoir_rows, decay, seed, update_interval=1, device=0):
        what = "SampleWindow"
        self.hist_size = _args.integer(hist_size, f"{what}: hist_size must be an integer >= 1, got {hist_size!r}", 1)
        self.reservoir_rows = _args.integer(reservoir_rows, f"{what}: reservoir_rows must be an integer in [0, 2^30], got {reservoir_rows!r}", 0, MAX_ROWS)
        self.decay = _args.unit_fraction(decay, f"{what}: decay must be a number in (0, 1], got {decay!r}")
        self.seed = _args.seed64(seed, what)
        self.update_interval = _args.integer(update_interval, f"{what}: update_interval must be an integer >= 1, got {update_interval!r}", 1)
        self.device = _args.device_index(device, what)
        self._window = []          # [(iteration, (canonical, v, pi))], ascending
        self._staged = []          # the same: evicted, not yet merged
        self._reservoir = None     # (canonical, v, pi, iterations int32, row ids int64)
        self._shapes = None
        self._newest_merged = -1   # the newest iteration that went into the reservoir
        self._evicted = 0
        self._syncs = 0
        self.last_update = None    # what the last merging update_reservoir saw: its pool and its choice

    def append(self, iteration, samples):
        """Keep the (canonical, v, pi) of `iteration` (CUDA tensors are kept as they are, numpy arrays are staged on the window's device);
        the iterations at or below iteration - hist_size move to staging."""
        what = "SampleWindow.append"
        iteration = _args.integer(iteration, f"{what}: iteration must be an integer in [0, 2^31), got {iteration!r}", 0, (1 << 31) - 1)
        kind, n, c, v, pi = _check_samples(what, samples, 1)
        newest = max([t for t, _ in self._window + self._staged] + [self._newest_merged])
        if iteration <= newest:
            raise RuntimeError(f"{what}: iterations are appended in ascending order, got {iteration} after {newest}")
        shapes = _row_shapes(what, c, v, pi)
        if self._shapes is not None and shapes != self._shapes:
            raise RuntimeError(f"{what}: rows of shapes {shapes} in a window of {self._shapes}")
        if kind == "numpy":
            c, v, pi = _stage(c, self.device), _stage(v, self.device), _stage(pi, self.device)
        elif c.device.index != self.device:
            raise RuntimeError(f"{what}: the samples are on {c.device}, the window on device {self.device}")
        self._shapes = shapes
        self._window.append((iteration, (c, v, pi)))
        while self._window and self._window[0][0] <= iteration - self.hist_size:
            self._staged.append(self._window.pop(0))
            self._evicted += 1

    def update_reservoir(self, iteration):
        """The merge of update_reservoir (game_runner.py:1815-1859) on one chunk: pool = reservoir + staging; while the pool has at
        most reservoir_rows rows it IS the new reservoir (the fill phase), otherwise the rows of the reservoir_rows largest
        reservoir_keys are kept, in pool order (select_top: the one synchronisation).  One gather per array.  Does nothing when
        iteration is no multiple of update_interval or nothing is staged.  -> the rows of the reservoir."""
        what = "SampleWindow.update_reservoir"
        iteration = _args.integer(iteration, f"{what}: iteration must be an integer in [0, 2^31), got {iteration!r}", 0, (1 << 31) - 1)
        if iteration % self.update_interval or not self._staged:
            return self.stats()["reservoir_rows"]
        import torch
        dev = torch.device("cuda", self.device)
        pool = ([(None, self._reservoir[:3])] if self._reservoir is not None else []) + self._staged
        if len(pool) > WINDOW_MAX_SEGMENTS:
            raise RuntimeError(f"{what}: {len(self._staged)} staged iterations: a pool holds at most {WINDOW_MAX_SEGMENTS} segments; "
                               "call update_reservoir more often")
        rows_list = [int(seg[0].shape[0]) for _, seg in pool]
        n = sum(rows_list)
        _check_rows(what, n)
        iters = [self._reservoir[3]] if self._reservoir is not None else []
        ids = [self._reservoir[4]] if self._reservoir is not None else []
        for t, seg in self._staged:
            rows = int(seg[0].shape[0])
            iters.append(torch.full((rows,), t, dtype=torch.int32, device=dev))
            ids.append(torch.arange(rows, dtype=torch.int64, device=dev) + (t << 32))
        iters, ids = torch.cat(iters), torch.cat(ids)
        self._newest_merged = max(self._newest_merged, self._staged[-1][0])
        self._staged = []
        if n == 0 or self.reservoir_rows == 0:
            return self.stats()["reservoir_rows"]
        keys = None
        if n > self.reservoir_rows:
            keys = reservoir_keys(iters, iteration, self.decay, _rng.mix64((self.seed + _GOLDEN * (iteration + 1)) & _rng.MASK64), row_ids=ids)
            index, _ = select_top(keys, self.reservoir_rows)
            self._syncs += 1
        else:
            index = torch.arange(n, dtype=torch.int64, device=dev)
        k = int(index.shape[0])
        kept = [_window_gather([seg[a] for _, seg in pool], rows_list, index, 0, 0, 0, k, None) for a in range(3)]
        kept += [_window_gather([x], [n], index, 0, 0, 0, k, None) for x in (iters, ids)]
        self._reservoir = tuple(kept)
        self.last_update = {"iteration": iteration, "pool_rows": n, "pool_iterations": iters, "pool_row_ids": ids, "keys": keys, "index": index}
        return k

    def segments(self):
        """the (canonical, v, pi) triples batches() reads: the window's iterations in ascending order, then the reservoir"""
        return [seg for _, seg in self._window] + ([self._reservoir[:3]] if self._reservoir is not None else [])

    def batches(self, batch_rows, sample_rate=1.0, pass_seed=0):
        """train()'s step budget (game_runner.py:1314-1317): ceil(average_generation / batch_rows * sample_rate) batches, where
        average_generation is the window's rows over its iterations, cut from shuffled passes over window + reservoir
        (window_batches; pass p is keyed by (pass_seed, p), a pass ends with a short batch and the next one begins).  -> a
        generator of (canonical, v, pi) CUDA batches; no synchronisation."""
        what = "SampleWindow.batches"
        batch_rows = _args.integer(batch_rows, f"{what}: batch_rows must be an integer in [1, 2^30], got {batch_rows!r}", 1, MAX_ROWS)
        sample_rate = _args.number(sample_rate, f"{what}: sample_rate must be a finite number >= 0, got {sample_rate!r}")
        pass_seed = _args.seed64(pass_seed, what)
        segs = self.segments()
        if len(segs) > WINDOW_MAX_SEGMENTS:
            raise RuntimeError(f"{what}: the window and the reservoir are {len(segs)} segments: at most {WINDOW_MAX_SEGMENTS}")
        rows_list = [int(seg[0].shape[0]) for seg in segs]
        window_rows = sum(rows_list[:len(self._window)])
        count = int(np.ceil(window_rows / len(self._window) / batch_rows * sample_rate)) if self._window else 0

        def run():
            left, p = count, 0
            while left > 0 and sum(rows_list) > 0:
                for batch in _pass_batches(segs, rows_list, batch_rows, pass_seed, p, 0, left, None):
                    left -= 1
                    yield batch
                p += 1
        return run()

    def newest(self):
        """(iteration, (canonical, v, pi)) of the newest iteration in the window, None for an empty window"""
        return self._window[-1] if self._window else None

    def stats(self):
        return {"window_rows": sum(int(seg[0].shape[0]) for _, seg in self._window),
                "reservoir_rows": 0 if self._reservoir is None else int(self._reservoir[0].shape[0]),
                "staged_rows": sum(int(seg[0].shape[0]) for _, seg in self._staged),
                "window_iterations": [t for t, _ in self._window],
                "evicted_iterations": self._evicted, "host_syncs": self._syncs}


# ---- the participation ratio: feature_rank, effective_rank ------------------------------------------------------------------------
def _check_features(what, features):
    """-> (kind, n, C) of a contiguous float32 [n, C] array, 1 <= C <= 2048"""
    kind = _kind(what, (("features", features),))
    shape = tuple(features.shape)
    if len(shape) != 2:
        raise RuntimeError(f"{what}: features must be an [n, C] array, got shape {shape}")
    n, Cn = int(shape[0]), int(shape[1])
    _check_rows(what, n)
    if not 1 <= Cn <= FEATURE_RANK_MAX_CHANNELS:
        raise RuntimeError(f"{what}: C must be in [1, {FEATURE_RANK_MAX_CHANNELS}], got {Cn}")
    _check_dtype(what, "features", features, "float32")
    return kind, n, Cn


def _rank_record(feats_t, mean_t, gram_t, stream):
    """azmi_samples_feature_rank on a float32 CUDA tensor [n, C] -> the record"""
    rec = FeatureRankRecordC()
    _call(lib.azmi_samples_feature_rank(feats_t.data_ptr(), int(feats_t.shape[0]), int(feats_t.shape[1]), None if mean_t is None else mean_t.data_ptr(),
                                        None if gram_t is None else gram_t.data_ptr(), C.byref(rec), feats_t.device.index,
                                        _stream_of(feats_t.device, stream)))
    return rec


def feature_rank(features, return_gram=False, return_mean=False, device=0, stream=None):
    """The participation ratio (sum s^2)^2 / sum s^4 of the singular values s of the column-centred `features` [n, C] (contiguous
    float32, C <= 2048), the last lines of NNWrapper.effective_rank (neural_net.py:867-873), without the SVD: with G = Fc^T Fc the two
    sums are tr G and the squared Frobenius norm of G (azmi_samples_feature_rank).  float64 on the float32 features, two passes
    (the column means, then the centred products); every sum in an order fixed by (n, C), so two calls return the same bits.
    -> {"rank", "trace" (= sum s^2), "frob2" (= sum s^4), "n", "channels"}, with return_mean "mean" (float64 [C]) and with
    return_gram "gram" (float64 [C, C]): numpy for a numpy array (staged on `device`), CUDA tensors for a CUDA tensor (used in
    place on `stream`).  frob2 == 0 exactly (one row, equal rows) gives rank 1.0; n == 0 gives NaN and touches no device.  One
    synchronisation, the record."""
    what = "feature_rank"
    kind, n, Cn = _check_features(what, features)
    if kind == "numpy":
        device = _args.device_index(device, what)
    if n == 0:
        out = {"rank": float("nan"), "trace": 0.0, "frob2": 0.0, "n": 0, "channels": Cn}
        if return_mean or return_gram:
            nan = lambda shape: np.full(shape, np.nan, np.float64)
            if kind == "torch":
                import torch
                nan = lambda shape: torch.full(shape, float("nan"), dtype=torch.float64, device=features.device)
            if return_mean:
                out["mean"] = nan((Cn,))
            if return_gram:
                out["gram"] = nan((Cn, Cn))
        return out
    feats = _stage(features, device) if kind == "numpy" else features
    import torch
    mean = _empty(Cn, torch.float64, feats.device, stream) if return_mean else None
    gram = _empty((Cn, Cn), torch.float64, feats.device, stream) if return_gram else None
    rec = _rank_record(feats, mean, gram, stream)
    out = {"rank": float(rec.rank), "trace": float(rec.trace), "frob2": float(rec.frob2), "n": int(rec.n), "channels": int(rec.channels)}
    if return_mean:
        out["mean"] = mean.cpu().numpy() if kind == "numpy" else mean
    if return_gram:
        out["gram"] = gram.cpu().numpy() if kind == "numpy" else gram
    return out


def effective_rank(canonical, net, batch_rows=65536):
    """NNWrapper.effective_rank(batch) (neural_net.py:826-873) on the device: the participation ratio of the pooled trunk
    activations of `net` (a HipLeafNet of precision="fp32", the tier whose arithmetic is the reference's eager fp32 module) over
    `canonical` [n, C, H, W] (contiguous float32; a numpy array is staged on the net's device, a CUDA tensor used in place).  The
    net's trunk runs over chunks of `batch_rows` rows into one [n, trunk_channels] float32 array (HipLeafNet.trunk_features), one
    feature_rank call follows.  -> a float in [1, trunk_channels]; NaN for None or an empty batch.  A HipLeafNet of another tier
    raises RuntimeError naming precision='fp32'.  The chunking does not change the bits.  One synchronisation, the record."""
    what = "effective_rank"
    batch_rows = _args.integer(batch_rows, f"{what}: batch_rows must be an integer >= 1, got {batch_rows!r}", 1)
    if canonical is None:
        return float("nan")
    kind = _kind(what, (("canonical", canonical),))
    shape = tuple(canonical.shape)
    if len(shape) != 4:
        raise RuntimeError(f"{what}: canonical must be an [n, C, H, W] array, got shape {shape}")
    n = int(shape[0])
    _check_rows(what, n)
    _check_dtype(what, "canonical", canonical, "float32")
    if not hasattr(net, "trunk_features"):
        raise RuntimeError(f"{what}: net must be a HipLeafNet, got {type(net).__name__}")
    cf = net.trunk_channels      # (raises for every tier but fp32, before anything is staged or launched)
    if n == 0:
        return float("nan")
    c = _stage(canonical, net.device) if kind == "numpy" else canonical
    import torch
    feats = torch.empty((n, cf), dtype=torch.float32, device=c.device)
    for lo in range(0, n, batch_rows):
        hi = min(n, lo + batch_rows)
        net.trunk_features(c[lo:hi], out=feats[lo:hi])
    return float(_rank_record(feats, None, None, None).rank)
