from deep_recommenders_amd.keras.models.nlp.bert import BERT, BertEmbedding, BertLayer, BertPretraining
from deep_recommenders_amd.keras.models.nlp.multi_head_attention import MultiHeadAttention
from deep_recommenders_amd.keras.models.nlp.transformer import Transformer
from deep_recommenders_amd.keras.models.nlp.word2vec import Word2Vec
