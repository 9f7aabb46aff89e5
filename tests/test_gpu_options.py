"""GPU (MI355X): what ppcsr_set_option accepts and refuses.  The checks are the ones tests/test_sim_options.py runs on the
emulator (tests/option_checks.py)."""
import pytest

import option_checks as oc
from helpers import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    pkg = load_pkg()
    pkg.load_library()  # must be the in-tree HIP build; raises if missing
    return lambda n: pkg.PCSR(n)


def test_option_return_codes(make):
    oc.return_codes(make)


def test_batch_after_option_calls(make, streams):
    oc.return_codes(make)
    oc.batch_after(make, {}, streams)
