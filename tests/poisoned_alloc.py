"""`poisoned_empty()`: every `torch.empty*` inside the block comes back filled with NaN (floating types) or the type's maximum (integer types).

A test process mostly sees freshly mapped device memory, which reads as zero; a training run sees recycled blocks of the caching allocator, full of the previous
tenant's values.  A kernel that accumulates into a workspace it takes for zero, skips an element of its output, or pairs a never-written pad lane with a zero
operand passes every finite-data test and corrupts a long run.  With the fill on, such a launch gives NaN where it gave the right number.

The fill is PyTorch's own: it is on while `torch.use_deterministic_algorithms(True, warn_only=True)` holds and `torch.utils.deterministic.fill_uninitialized_memory`
is true.  Deterministic mode may also choose other aten algorithms, so wrap only the product call under test, never the float64 reference or input generation.
"""

import contextlib

import torch


@contextlib.contextmanager
def poisoned_empty():
    det = torch.are_deterministic_algorithms_enabled()
    warn_only = torch.is_deterministic_algorithms_warn_only_enabled()
    fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(det, warn_only=warn_only)
        torch.utils.deterministic.fill_uninitialized_memory = fill


FLOAT_TYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64)
INT_TYPES = (torch.uint8, torch.int32, torch.int64)


def _makers(device):
    like = lambda dt: torch.zeros([3, 5], dtype=dt, device=device)
    return {'empty': lambda dt: torch.empty([3, 5], dtype=dt, device=device),
            'empty_like': lambda dt: torch.empty_like(like(dt)),
            'new_empty': lambda dt: like(dt).new_empty([7, 2]),
            'empty_strided': lambda dt: torch.empty_strided([3, 5], [8, 1], dtype=dt, device=device)}


def check_fill(device):
    """Under the manager the four allocation calls give all-NaN / all-max tensors on `device`; the flags are restored afterwards, also after an exception."""
    for det, warn_only, fill in ((False, False, True), (False, False, False), (True, True, False), (True, False, True)):
        before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
                  torch.utils.deterministic.fill_uninitialized_memory)
        torch.use_deterministic_algorithms(det, warn_only=warn_only)
        torch.utils.deterministic.fill_uninitialized_memory = fill
        try:
            state = lambda: (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
                             torch.utils.deterministic.fill_uninitialized_memory)
            with poisoned_empty():
                assert state() == (True, True, True)
                for name, make in _makers(device).items():
                    for dt in FLOAT_TYPES:
                        t = make(dt)
                        assert t.dtype == dt and t.device.type == torch.device(device).type
                        assert bool(torch.isnan(t).all()), f'{name} {dt} on {device} is not all NaN'
                    for dt in INT_TYPES:
                        t = make(dt)
                        assert bool((t == torch.iinfo(dt).max).all()), f'{name} {dt} on {device} is not all max'
            assert state() == (det, warn_only, fill)
            try:
                with poisoned_empty():
                    raise KeyError('body')
            except KeyError:
                pass
            assert state() == (det, warn_only, fill), 'the flags were not restored after an exception'
        finally:
            torch.use_deterministic_algorithms(before[0], warn_only=before[1])
            torch.utils.deterministic.fill_uninitialized_memory = before[2]
