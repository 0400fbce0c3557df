"""What the bench tools of the meters and their stages share."""
import ctypes
import statistics


def median_ms(torch, stream, call, calls, warmup, before=None):
    """before: enqueued in front of every call, outside its pair of events"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            if before:
                before()
            call()
        for a, b in ev:
            if before:
                before()
            a.record(stream)
            call()
            b.record(stream)
    stream.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return statistics.median(ms), ms[0], ms[-1]


def loaded_hip_runtime():
    """The HIP runtime this process has already mapped (torch's and the library's one), opened by the path it was loaded
    from: the same handle, never a second copy under another name."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if len(paths) != 1:
        raise RuntimeError(f"expected one HIP runtime in the process, found {sorted(paths)}")
    return ctypes.CDLL(paths.pop())


def copy_call(dst, src, nbytes, s):
    """-> a call that enqueues a device-to-device hipMemcpyAsync of nbytes from src to dst (device addresses) on stream s"""
    hip = loaded_hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    def run_copy():
        if hip.hipMemcpyAsync(dst, src, nbytes, 3, s) != 0:      # 3: hipMemcpyDeviceToDevice
            raise RuntimeError("hipMemcpyAsync failed")

    return run_copy
