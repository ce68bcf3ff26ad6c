# same exports as the reference's keras/models/ranking/__init__.py:4-6
from deep_recommenders_amd.keras.models.ranking.fm import FM
from deep_recommenders_amd.keras.models.ranking.fm import FactorizationMachine
from deep_recommenders_amd.keras.models.ranking.deepfm import DeepFM
from deep_recommenders_amd.keras.models.ranking.xdeepfm import CINNetwork
from deep_recommenders_amd.keras.models.ranking.xdeepfm import XDeepFM
from deep_recommenders_amd.keras.models.ranking.dlrm import DotInteraction
from deep_recommenders_amd.keras.models.ranking.dlrm import DLRM
from deep_recommenders_amd.keras.models.ranking.afm import AttentionalPooling
from deep_recommenders_amd.keras.models.ranking.afm import AFM
from deep_recommenders_amd.keras.models.ranking.ffm import FieldAwareInteraction
from deep_recommenders_amd.keras.models.ranking.ffm import FFM
from deep_recommenders_amd.keras.models.ranking.dien import GRU
from deep_recommenders_amd.keras.models.ranking.dien import AUGRU
from deep_recommenders_amd.keras.models.ranking.dien import InterestExtractor
from deep_recommenders_amd.keras.models.ranking.dien import InterestEvolution
from deep_recommenders_amd.keras.models.ranking.dien import DIEN
