"""Does a captured hipMemsetAsync replay with the bytes it was given?  The runtime call alone, through ctypes, no project code:
a buffer of 0xEE, ONE hipMemsetAsync(p, 0xFF, n) captured with torch.cuda.graph on a side stream, one replay, the histogram of the
buffer.  Expected {255: n}.  On MI355X (torch 2.10 + its HIP 7.0.51831 runtime, ROCm 7.2.0 installed): {0: n} at 3 674 160 bytes and a mix of 0 and stale values at 65 536 -- why
rc_search.hip clears its tables with k_fill16.  Also with a kernel in front of the memset (x.add_), as a library launch inside a
larger captured step has.  Prints one line per case; nothing loops, nothing waits.

    python tools/probe_graph_memset.py
"""
import ctypes

import torch

hip = ctypes.CDLL("libamdhip64.so.7")      # the soname torch has loaded: one runtime in the process, as the libraries link it
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]


def histogram(t):
    v, c = torch.unique(t, return_counts=True)
    return dict(zip(v.tolist(), c.tolist()))


def case(name, n, kernel_first):
    buf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    x = torch.zeros(1024, device="cuda")
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            if kernel_first:
                x.add_(1.0)
            rc = hip.hipMemsetAsync(buf.data_ptr(), 0xFF, n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured = histogram(buf)
    g.replay()
    torch.cuda.synchronize()
    got = histogram(buf)
    print(f"{name}: rc {rc}; after capture {captured}; after replay {got}; {'ok' if got == {255: n} else 'WRONG'}", flush=True)


if __name__ == "__main__":
    print("torch", torch.__version__, "hip", torch.version.hip, torch.cuda.get_device_name(0))
    for n in (65536, 3674160):
        case(f"memset alone, {n} bytes", n, False)
        case(f"kernel, then memset, {n} bytes", n, True)
