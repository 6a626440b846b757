from .decentralized_lqr import DecentralizedLQR  # noqa: F401
from .decentralized_lqr_omega import DecentralizedLQROmega  # noqa: F401
