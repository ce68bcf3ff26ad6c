"""Word2Vec: skip-gram with negative sampling under the name the reference's README uses (it lists the model and ships no code).
The model, its kernels and its training step are SkipGram's (keras/models/retrieval/skipgram.py): `counts` are the corpus word counts
(negatives follow counts ** 0.75), layers.skipgram_pairs turns padded sentences into (center, context) pairs."""
from deep_recommenders_amd.keras.models.retrieval.skipgram import SkipGram


class Word2Vec(SkipGram):
    pass
