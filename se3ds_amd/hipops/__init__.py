"""Host-side wrappers of the libse3ds_hip.so network kernels: a small reverse-mode tape
(gradient accumulation runs in our own kernels, not in torch) and the differentiable ops the
SE3DS layers are written with."""
