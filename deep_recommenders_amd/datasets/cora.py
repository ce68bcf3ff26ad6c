"""Cora citation graph -- same surface as the reference's datasets/cora.py:8-126 (load_content, build_graph, spectral_graph,
sample_train_nodes, encode_labels, split_labels, num_classes), host-side numpy / scipy like the reference.  There is no download:
the files must already be at <extract_path>/cora/ (FileNotFoundError names the archive to fetch by hand).

synthetic_cora() writes a seeded Cora-shaped planted-partition graph in the same two-file format, for machines without the data."""
import os

import numpy as np
import scipy.sparse as sp

CORA_URL = "https://linqs-data.soe.ucsc.edu/public/lbc/cora.tgz"
CORA_CLASSES = ["Case_Based", "Genetic_Algorithms", "Neural_Networks", "Probabilistic_Methods", "Reinforcement_Learning",
                "Rule_Learning", "Theory"]


class Cora(object):

    def __init__(self, extract_path="."):
        self._download_url = CORA_URL
        self._extract_path = extract_path
        self._cora_path = os.path.join(extract_path, "cora")
        self._cora_cites = os.path.join(self._cora_path, "cora.cites")
        self._cora_content = os.path.join(self._cora_path, "cora.content")
        if not os.path.exists(self._cora_cites) or not os.path.exists(self._cora_content):
            # the reference downloads here (cora.py:17-19); this package never touches the network
            raise FileNotFoundError("Cora files not found under %s: fetch %s by hand and extract it there (cora/cora.cites, "
                                    "cora/cora.content)" % (os.path.abspath(self._cora_path), self._download_url))
        self._cora_classes = list(CORA_CLASSES)

    @property
    def num_classes(self):
        return len(self._cora_classes)

    def load_content(self, normalize=True):
        content = np.genfromtxt(self._cora_content, dtype=str)
        ids, features, labels = content[:, 0], content[:, 1:-1], content[:, -1]
        features = sp.csr_matrix(features, dtype=np.float32)
        if normalize is True:           # features / row sums (cora.py:52-53), kept sparse
            s = np.asarray(features.sum(axis=1), dtype=np.float32).reshape(-1)
            with np.errstate(divide="ignore"):
                inv = np.float32(1.0) / s
            features = sp.csr_matrix(sp.diags(inv) @ features, dtype=np.float32)
        return ids, features, labels

    def build_graph(self, nodes):
        idx_map = {int(j): i for i, j in enumerate(nodes)}
        edges_unordered = np.genfromtxt(self._cora_cites, dtype=np.int32).reshape(-1, 2)
        edges = np.array(list(map(idx_map.get, edges_unordered.flatten())),
                         dtype=np.int32).reshape(edges_unordered.shape)
        graph = sp.coo_matrix((np.ones(edges.shape[0]), (edges[:, 0], edges[:, 1])),
                              shape=(nodes.shape[0], nodes.shape[0]), dtype=np.float32)
        graph += graph.T - sp.diags(graph.diagonal())  # Convert symmetric matrix
        return graph

    @staticmethod
    def spectral_graph(graph):
        graph = graph + sp.eye(graph.shape[0])  # graph G with added self-connections
        # D^{-1/2} * A * D^{-1/2}
        d = sp.diags(np.power(np.array(graph.sum(1)), -0.5).flatten(), 0)
        spectral_graph = graph.dot(d).transpose().dot(d).tocsr()
        return spectral_graph

    def sample_train_nodes(self, labels, num_per_class=20):
        train_nodes = []
        for cls in self._cora_classes:
            cls_index = np.where(labels == cls)[0]
            cls_sample = np.random.choice(cls_index, num_per_class, replace=False)
            train_nodes += cls_sample.tolist()
        return train_nodes

    def encode_labels(self, labels):
        labels_map = {}
        num_classes = len(self._cora_classes)
        for i, cls in enumerate(self._cora_classes):
            cls_label = np.zeros(shape=(num_classes,))
            cls_label[i] = 1.
            labels_map[cls] = cls_label
        encoded_labels = list(map(labels_map.get, labels))
        return np.array(encoded_labels, dtype=np.int32)

    def split_labels(self, labels, num_valid_nodes=500):
        num_nodes = labels.shape[0]
        all_index = np.arange(num_nodes)
        train_index = self.sample_train_nodes(labels)
        valid_index = list(set(all_index) - set(train_index))
        valid_index, test_index = valid_index[:num_valid_nodes], valid_index[num_valid_nodes:]

        encoded_labels = self.encode_labels(labels)

        def _sample_mask(index_ls):
            mask = np.zeros(num_nodes)
            mask[index_ls] = 1
            return np.array(mask, dtype=bool)

        def _get_labels(index_ls):
            _labels = np.zeros(encoded_labels.shape, dtype=np.int32)
            _labels[index_ls] = encoded_labels[index_ls]
            _mask = _sample_mask(index_ls)
            return _labels, _mask

        train_labels, train_mask = _get_labels(train_index)
        valid_labels, valid_mask = _get_labels(valid_index)
        test_labels, test_mask = _get_labels(test_index)

        return (train_labels, train_mask), \
               (valid_labels, valid_mask), \
               (test_labels, test_mask)


def synthetic_cora(extract_path, num_nodes=2708, num_features=1433, num_edges=5429, words_per_node=18, p_in=0.9, seed=0):
    """Writes <extract_path>/cora/cora.{content,cites}: a seeded planted-partition graph of Cora's shape (7 classes, sparse binary
    bag-of-words features with a class-dependent vocabulary, citations mostly inside a class).  Returns extract_path."""
    r = np.random.RandomState(seed)
    C = len(CORA_CLASSES)
    labels = r.randint(0, C, size=num_nodes)
    ids = r.choice(np.arange(1, 10 * num_nodes), size=num_nodes, replace=False)
    vocab = np.array_split(r.permutation(num_features), C)          # each class favours its own slice of the vocabulary
    rows = []
    for i in range(num_nodes):
        own = r.choice(vocab[labels[i]], size=words_per_node // 2, replace=False)
        other = r.choice(num_features, size=words_per_node - words_per_node // 2, replace=False)
        f = np.zeros(num_features, dtype=np.int8)
        f[own] = 1
        f[other] = 1
        rows.append(f)
    by_class = [np.where(labels == c)[0] for c in range(C)]
    src = r.randint(0, num_nodes, size=num_edges)
    dst = np.empty(num_edges, dtype=np.int64)
    for e in range(num_edges):
        if r.rand() < p_in:
            dst[e] = r.choice(by_class[labels[src[e]]])
        else:
            dst[e] = r.randint(0, num_nodes)
    path = os.path.join(extract_path, "cora")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "cora.content"), "w") as f:
        for i in range(num_nodes):
            f.write("%d\t%s\t%s\n" % (ids[i], "\t".join(map(str, rows[i])), CORA_CLASSES[labels[i]]))
    with open(os.path.join(path, "cora.cites"), "w") as f:
        for s, d in zip(src, dst):
            f.write("%d\t%d\n" % (ids[d], ids[s]))
    return extract_path
