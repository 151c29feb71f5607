"""What the CPU tests of the fcnet C surface (tests/test_actor_cpu.py ... tests/test_learner_group_accum_cpu.py) share: the return
codes, the library fixture, the fake-pointer images of the batch and hyper structs, the header-member parser and the two gcc runners.
No GPU and no handle: a pointer here is the number 4096 and is never dereferenced by the checks under test."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, 'include')
OK, EINVAL, EUNSUPPORTED, EABI = 0, -1, -6, -7
C99 = ['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE]


@pytest.fixture(scope='module')
def lib():
    from deepcomp_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 on a GPU-less host
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------ fake-pointer structs
# the pointer members behind the scalars, in each header's order
PPO_FIELDS = ('obs', 'actions', 'old_logp', 'old_logits', 'advantages', 'value_targets', 'old_vf', 'logp', 'entropy', 'kl', 'vf', 'ratio', 'dlogits', 'dvalue')
SGD_FIELDS = ('obs', 'actions', 'old_logp', 'old_logits', 'advantages', 'value_targets', 'old_vf', 'dlogits', 'dvalue', 'logp', 'entropy', 'kl', 'vf', 'ratio')
LOSS_INPUTS = PPO_FIELDS[:7]


def _size(struct, size):
    return ctypes.sizeof(struct) if size is None else size


def ppo_batch(given=LOSS_INPUTS, size=None, fmt=0, rows=8, num_active=1):
    from deepcomp_amd import _lib
    return _lib.DcompPpoBatch(_size(_lib.DcompPpoBatch, size), fmt, rows, num_active, 0, *[4096 if n in given else None for n in PPO_FIELDS])


def sgd_batch(given=LOSS_INPUTS, size=None, fmt=0, rows=8, source_rows=64, index=4096, num_active=1):
    from deepcomp_amd import _lib
    return _lib.DcompSgdBatch(_size(_lib.DcompSgdBatch, size), fmt, rows, source_rows, index, num_active, 0,
                              *[4096 if n in given else None for n in SGD_FIELDS])


def group_batch(rows=None, size=None, stride=64, index=4096, given=True, source_rows=640):
    from deepcomp_amd import _lib
    ptr = 4096 if given else None
    arr = (ctypes.c_int64 * len(rows))(*rows) if rows is not None else None
    b = _lib.DcompGroupBatch(_size(_lib.DcompGroupBatch, size), 0, source_rows, ptr, ptr, ptr, ptr, ptr, ptr, ptr, index, stride, arr)
    b._keep = arr
    return b


def ppo_hyper(size=None, clip=0.3, vf_clip=10.0):
    from deepcomp_amd import _lib
    return _lib.DcompPpoHyper(_size(_lib.DcompPpoHyper, size), clip, vf_clip, 1.0, 0.0, 0.2)


def ppo_hypers(P, size=None, bad=None):
    """An array of P hypers; bad: the entry whose struct_size is `size`."""
    from deepcomp_amd import _lib
    hy = (_lib.DcompPpoHyper * P)(*[ppo_hyper() for _ in range(P)])
    if bad is not None:
        hy[bad].struct_size = size
    return hy


# ------------------------------------------------------------------------------------------------------------ headers
def header(name):
    return os.path.join(INCLUDE, name)


def struct_members(path, cname):
    """The member names of `typedef struct cname { ... } cname;` in a header, in order, from its text."""
    txt = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), txt, flags=re.S).group(1)
    return [re.split(r'[\s*]+', m.strip())[-1] for decl in body.split(';') if decl.strip() for m in decl.split(',')]


def compiles_as_c99(tmp_path, stem, texts):
    """Every text of `texts` as a translation unit of its own through gcc -std=c99 -Wall -Wextra -Werror -pedantic -fsyntax-only:
    a header alone, behind the others, in front of them."""
    for n, text in enumerate(texts):
        src = tmp_path / f'{stem}{n}.c'
        src.write_text(text)
        subprocess.run(C99 + ['-fsyntax-only', str(src)], check=True)


def c_program_output(tmp_path, text, link=()):
    """`text` compiled as C99 (pedantic, warnings are errors), linked and run: the integers it prints, one list per line."""
    src, exe = tmp_path / 'sizes.c', tmp_path / 'sizes'
    src.write_text(text)
    subprocess.run(C99 + ['-fsyntax-only', str(src)], check=True)
    subprocess.run(['gcc', '-std=c99', '-I', INCLUDE, *link, '-o', str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.strip()
    return [[int(x) for x in line.split()] for line in out.split('\n')]
