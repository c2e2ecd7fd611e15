"""rroi_align._ext -- ctypes binding of librroi_align_hip.so: the package `rroi_align`, one module per operator (see its
__init__.py)."""
