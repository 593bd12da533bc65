"""Recorded calls of the reference's own kernels (oracle/ref.py over oracle/_ref), for hosts without them.

tests/test_oracle_ref.py compares the oracle with the reference's gradient kernel and forward data movers, compiled
for the host from the reference's sources.  Where those sources are absent its `ref` fixture is a `Replay`: the same
functions, answering from tests/golden/ref_recorded/calls_*.npz, which hold what the reference kernels returned for every input
those tests pass them.  A call is looked up by the sha256 of its exact arguments (dtype, shape and bytes), so a replayed
result is never paired with inputs other than the ones it was computed from; an input that is not recorded (the
full-size K3 scene, whose outputs are too large to commit, or scene arrays that a host's floating-point library
builds differently) skips the test with that reason.

Regenerate where the reference is present:  python -m tests.golden.ref_calls
(runs tests/test_oracle_ref.py with a `Recorder` around oracle/ref.py and rewrites the files).
"""
import glob
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = os.path.join(HERE, 'ref_recorded', 'calls_%d.npz')
SHARDS = 3                       # the calls are spread over this many files, balanced by size (each well under 1 MiB)
RECORD_ENV = 'DIRT_RECORD_REF_CALLS'
MAX_RECORDED_BYTES = 512 << 10   # per call: a larger result (the K3 scene) is not recorded
FUNCTIONS = ('backward', 'forward', 'upload_vertices', 'atlas_shape')


def call_key(name, args):
    h = hashlib.sha256(name.encode())
    for a in args:
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            h.update(('%s%s' % (a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
        else:
            h.update(repr(a).encode())
    return name + '-' + h.hexdigest()[:32]


def _nbytes(result):
    if isinstance(result, dict):
        return sum(np.asarray(v).nbytes for v in result.values())
    return np.asarray(result).nbytes


class Recorder:
    """oracle/ref.py with every call of FUNCTIONS also kept (key -> result) for `save`."""

    def __init__(self, module):
        self._module = module
        self.calls = {}

    def __getattr__(self, name):
        fn = getattr(self._module, name)
        if name not in FUNCTIONS:
            return fn

        def recorded(*args):
            result = fn(*args)
            if _nbytes(result) <= MAX_RECORDED_BYTES:
                self.calls[call_key(name, args)] = result
            return result
        return recorded

    def save(self):
        os.makedirs(os.path.dirname(PATHS), exist_ok=True)
        for old in glob.glob(PATHS.replace('%d', '*')):
            os.remove(old)
        shards = [{} for _ in range(SHARDS)]
        sizes = [0] * SHARDS
        for key, result in sorted(self.calls.items(), key=lambda kv: (-_nbytes(kv[1]), kv[0])):
            i = sizes.index(min(sizes))
            sizes[i] += _nbytes(result)
            if isinstance(result, dict):
                for k, v in result.items():
                    shards[i][key + '/' + k] = np.asarray(v)
            else:
                shards[i][key] = np.asarray(result)
        for i, members in enumerate(shards):
            np.savez_compressed(PATHS % i, **members)


def recorded():
    return all(os.path.exists(PATHS % i) for i in range(SHARDS))


class Replay:
    """The FUNCTIONS of oracle/ref.py, answered from the recorded calls."""

    def __init__(self):
        self._where = {}
        for i in range(SHARDS):
            z = np.load(PATHS % i, allow_pickle=False)
            self._where.update((name, z) for name in z.files)

    def _lookup(self, name, args):
        import pytest
        key = call_key(name, args)
        if key in self._where:
            return self._where[key][key]
        fields = [n for n in self._where if n.startswith(key + '/')]
        if not fields:
            pytest.skip('the reference kernels are not built here and this input is not among the recorded calls '
                        '(tests/golden/ref_recorded/)')
        return {n.split('/', 1)[1]: self._where[n][n] for n in fields}

    def backward(self, *args):
        return self._lookup('backward', args)

    def forward(self, *args):
        return self._lookup('forward', args)

    def upload_vertices(self, *args):
        return self._lookup('upload_vertices', args)

    def atlas_shape(self, *args):
        return tuple(int(x) for x in self._lookup('atlas_shape', args))


def main():
    import pytest
    from oracle import ref
    if not ref.available():
        raise SystemExit('oracle/_ref cannot be built here: the reference kernels are needed to record their calls')
    os.environ[RECORD_ENV] = '1'
    test = os.path.join(os.path.dirname(HERE), 'test_oracle_ref.py')
    rc = pytest.main(['-q', '-p', 'no:cacheprovider', test])
    if rc != 0:
        raise SystemExit('tests/test_oracle_ref.py failed while recording (%d)' % rc)
    for i in range(SHARDS):
        print('wrote', PATHS % i, '%d bytes' % os.path.getsize(PATHS % i), file=sys.stderr)


if __name__ == '__main__':
    main()
