from . import hais                                             # noqa: F401
from .hais import HAIS                                         # noqa: F401
