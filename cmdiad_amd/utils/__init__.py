def gpu_device(device, message):
    """The current device (after selecting ``device`` when one is given) for a module without a CPU path; NativeError(message)
    where there is no GPU."""
    import torch
    from .. import _native as nat
    if not torch.cuda.is_available():
        raise nat.NativeError(message)
    if device is not None:
        torch.cuda.set_device(int(device))      # the kernels are enqueued on the current device's current stream
    return torch.device("cuda", torch.cuda.current_device())
