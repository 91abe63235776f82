"""The layer chain of the glimpse VAE (reference air/vae.py:5-43) as a table -- pure host code.

The chain is rec<i> ... -> ml -> gen<i> ... -> out: `ml` is rec_mean | rec_log_variance as ONE fused [K, 2Z] product, `out`
is gen_mean.  The widths run d -> rec... -> 2Z and Z -> gen... -> d.  VariableStore, air.vae.VAE and the launch-list builders
of AIRModel read this table; it knows nothing about buffers, twins or precision."""
from collections import OrderedDict, namedtuple

import numpy as np
import torch

# one product y = x . W + b: the fused names of W [K, N] and b [N]
Product = namedtuple("Product", "w b K N")


class VaeLayers:
    def __init__(self, input_dim, rec_units, latent_dim, gen_units):
        d, Z = int(input_dim), int(latent_dim)
        self.input_dim, self.latent_dim = d, Z

        def chain(stem, k, units):
            out = []
            for i, u in enumerate(units):
                out.append(Product("%s%d_w" % (stem, i), "%s%d_b" % (stem, i), k, int(u)))
                k = int(u)
            return out, k
        self.rec, k = chain("rec", d, rec_units)
        self.ml = Product("ml_w", "ml_b", k, 2 * Z)
        self.gen, k = chain("gen", Z, gen_units)
        self.out = Product("out_w", "out_b", k, d)
        # encoder[0] reads the input and encoder[i + 1] the activation of rec[i]; decoder[0] reads the sample z and
        # decoder[i + 1] the activation of gen[i]
        self.encoder, self.decoder = self.rec + [self.ml], self.gen + [self.out]

    def products(self):
        """every product, in layer order (the creation order of the variables)"""
        return self.encoder + self.decoder

    def shapes(self):
        """fused name -> shape, in creation order"""
        out = OrderedDict()
        for l in self.products():
            out[l.w], out[l.b] = (l.K, l.N), (l.N,)
        return out

    @staticmethod
    def tf_names_of(n_rec, n_gen):
        """the TF variable names of vae.py under the scope vae/, in creation order, for that many hidden layers"""
        layers = ["recognition_%d" % (i + 1) for i in range(n_rec)] + ["rec_mean", "rec_log_variance"] + \
                 ["generative_%d" % (i + 1) for i in range(n_gen)] + ["gen_mean"]
        return ["vae/%s/%s" % (layer, kind) for layer in layers for kind in ("weights", "biases")]

    def tf_names(self):
        return self.tf_names_of(len(self.rec), len(self.gen))

    def tf_views(self, V):
        """TF name -> view of the fused-name mapping V (rec_mean / rec_log_variance: the column halves of ml_w / ml_b)"""
        Z, names = self.latent_dim, iter(self.tf_names())
        # (product, its columns or None for all of them) per TF layer, in the order of the names
        layers = [(l, None) for l in self.rec] + [(self.ml, slice(0, Z)), (self.ml, slice(Z, 2 * Z))] + \
                 [(l, None) for l in self.gen] + [(self.out, None)]
        out = OrderedDict()
        for l, cols in layers:
            out[next(names)] = V[l.w] if cols is None else V[l.w][:, cols]
            out[next(names)] = V[l.b] if cols is None else V[l.b][cols]
        return out


def load_variables(mine, mapping, scope=""):
    """Copies every variable of the name -> tensor mapping `mine` from mapping[scope + name] (tensors or arrays).  All of
    them must be there with the right number of elements: nothing is written otherwise."""
    prefix = scope if (not scope or scope.endswith("/")) else scope + "/"
    src = {}
    for name, v in mine.items():
        if prefix + name not in mapping:
            raise KeyError("missing variable %s" % (prefix + name))
        t = mapping[prefix + name]
        t = t.detach() if torch.is_tensor(t) else torch.as_tensor(np.array(t))
        if t.numel() != v.numel():
            raise ValueError("variable %s has %r elements, expected %r" % (prefix + name, tuple(t.shape), tuple(v.shape)))
        src[name] = t
    with torch.no_grad():
        for name, v in mine.items():
            v.copy_(src[name].to(device=v.device, dtype=v.dtype).reshape(v.shape))
