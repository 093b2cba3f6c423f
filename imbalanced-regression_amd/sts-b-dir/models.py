"""Drop-in for the head of the reference's ``sts-b-dir/models.py``: ``from models import PairHead, pair_tail_forward``. It covers
``HeadlessPairEncoder.forward`` from the second dropout on (models.py:155-166: dropout on the two LSTM encodings, padding to -inf, max
over time, ``cat[u, v, |u - v|, u * v]``) and ``MultiTaskModel.forward`` (models.py:84-114: ``FDS.smooth``, the ``Linear(4 * d_pair, 1)``
regressor, the weighted loss on ``label / 5``) as one fused HIP head. The text-field embedder, the highway layers, the BiLSTM
(models.py:137-153), ``build_model`` / ``build_regressor`` and the AllenNLP trainer stay with the reference (out of scope);
the scorer call of models.py:109-111 is ``util.STSShotAverage``."""
import _path  # noqa: F401
from dirhip.pair_tail import PairHead, pair_tail_forward  # noqa: F401
