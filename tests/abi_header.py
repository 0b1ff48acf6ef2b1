"""include/segan_hip.h, read once for the tests that pin it.  Its own small regexes, on purpose
independent of the reader in segan_pytorch_amd/_lib.py that the binding is derived with."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'include', 'segan_hip.h')) as _f:
    RAW = _f.read()                                     # the file, comments included
CODE = re.sub(r'/\*.*?\*/', '', RAW, flags=re.S)        # without its comments


def args(name, ret='int'):
    """The arguments of the declaration ``<ret> <name>(...)`` as a list of strings."""
    m = re.search(r'\b' + ret + ' ' + name + r'\s*\(([^)]*)\)', CODE)
    assert m, name
    return m.group(1).split(',')


def macro(name):
    """The integer a ``#define <name> <integer>`` line gives."""
    m = re.search(r'#define {} (-?\d+)\b'.format(name), CODE)
    assert m, name
    return int(m.group(1))
