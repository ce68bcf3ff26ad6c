# same exports as the reference's keras/models/retrieval/__init__.py
from deep_recommenders_amd.keras.models.retrieval.factorized_top_k import FactorizedTopK
from deep_recommenders_amd.keras.models.retrieval.gcn import GCN
# listed in the reference's README, no code there
from deep_recommenders_amd.keras.models.retrieval.skipgram import SkipGram
from deep_recommenders_amd.keras.models.retrieval.skipgram import Item2Vec
from deep_recommenders_amd.keras.models.retrieval.skipgram import DeepWalk
from deep_recommenders_amd.keras.models.retrieval.youtubenet import YoutubeNet
from deep_recommenders_amd.keras.models.retrieval.ebr import EBR
from deep_recommenders_amd.keras.models.retrieval.eges import EGES
from deep_recommenders_amd.keras.models.retrieval.eges import graph_from_sessions
from deep_recommenders_amd.keras.models.retrieval.airbnb import Airbnb
from deep_recommenders_amd.keras.models.retrieval.graphsage import SAGEConv
from deep_recommenders_amd.keras.models.retrieval.graphsage import GraphSAGE
from deep_recommenders_amd.keras.models.retrieval.graphsage import PinSage
from deep_recommenders_amd.keras.models.retrieval.intentgc import IntentConv
from deep_recommenders_amd.keras.models.retrieval.intentgc import IntentNet
from deep_recommenders_amd.keras.models.retrieval.intentgc import IntentGC
from deep_recommenders_amd.keras.models.retrieval.intentgc import translate_relations
